"""Numpy specification of the fused bf16 attention strips (csrc/attn_b16.hip: sumk_attn_strips_b16), stage by stage, and the gates the GPU
test (tests/test_gpu_attn_strip.py) and the host test (tests/test_attn_strip_host.py) share.  TEST INFRASTRUCTURE ONLY.

Forward, per video of T frames, from bf16-valued Q, K, V (held as float32 arrays):
  alpha = softmax_j(masked_logit(Q K^T * scale))       the mask rule of csrc/sumk_internal.h masked_logit (vasnet.py:119-127)
  keep  = dropout_keep(seed, 0, (packed_row << 20) | key, p)      tests/golden/recipes.py
  P     = bf16(keep ? alpha / (1 - p) : 0),  CTX = P V
Backward, from dCTX, V, K, alpha and the mask:
  d = keep ? (dCTX V^T) / (1 - p) : 0,  dS = scale * alpha * (d - sum_j d_j alpha_j),  dQ = bf16(dS) K
Every function is generic in `dtype`.  The float64 run is the reference (tests/test_attn_strip_host.py pins it to oracle/torch_port's VASNet
attention and to torch autograd).  The float32 run is the YARDSTICK: its products walk k in ascending order with one accumulator per
element, every product and every add rounded to float32 (`chain`, the rule oracle/torch_port.mm_chain states for an fp32-accumulating GEMM).

The kernel is held stage by stage, so that no stage's rounding is amplified by the next: E against alpha(Q, K); P16 bit for bit against
bf16_rne of the kernel's own E; O16 against the product of the kernel's own P16; in the backward P16 (bf16 dS) against dS of the E it was
given, and O16 (dQ) against the product of its own P16.  `model32` plays the kernel with the float32 specification (and, with `mutant`, with one
deliberate mistake): the host test proves that the gates accept the former and reject every one of the latter."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import recipes as R  # noqa: E402

MULT = 4.0
MUTANTS = ("drop_last_key_tile", "swap_p_chunks", "local_dropout_row", "no_max_subtraction", "pad_column_nonzero", "bf16_truncation")


# ---------------------------------------------------------------------------------------------------------------- bf16
def bf16_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (NaN -> a quiet NaN)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    out = ((u + ((u >> np.uint64(16)) & np.uint64(1)) + np.uint64(0x7FFF)) >> np.uint64(16)).astype(np.uint16)
    out[np.isnan(x)] = 0x7FC0
    return out


def bf16_bits_trunc(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    """uint16 bf16 bit patterns -> float32 values."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(np.asarray(x, dtype=np.float32)))


def bf16_half_spacing(x):
    """Half the distance between neighbouring bf16 values at |x| (float64), |x| floored at 2^-126."""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 0.5 * 2.0 ** (np.floor(np.log2(a)) - 7.0)


# ---------------------------------------------------------------------------------------------------------------- specification
def chain(a, b):
    """a (M, K) @ b (K, N) with one accumulator per element, k ascending, in the operands' dtype."""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=a.dtype)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * b[None, k, :]
    return acc


def matmul(a, b, dtype):
    f = np.dtype(dtype).type
    a, b = np.asarray(a).astype(f), np.asarray(b).astype(f)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return chain(a, np.ascontiguousarray(b)) if f is np.float32 else a @ b


def masked_logits(s, scale, ignore_self, aperture):
    """masked_logit of csrc/sumk_internal.h on a (T, T) block of raw logits, in s.dtype; aperture < 0: no band."""
    T = s.shape[0]
    e = s * s.dtype.type(np.float32(scale))
    i, j = np.ogrid[:T, :T]
    if ignore_self:
        e = np.where(i == j, -np.inf, e)
    if aperture >= 0:
        with np.errstate(under="ignore", invalid="ignore", over="ignore"):
            lo = np.where(j - i <= aperture, e, 0.0)
            up = np.where(j - i >= -aperture, e, 0.0)
            e = np.where(lo * up == 0.0, -np.inf, e)
    return e.astype(s.dtype)


def softmax_rows(e, max_subtraction=True, drop_keys=None):
    """Row softmax in e.dtype; a row without a finite logit is NaN.  (drop_keys: a mutant's excluded (rows, keys) block.)"""
    f = e.dtype.type
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        if drop_keys is not None:
            e = e.copy()
            e[drop_keys] = -np.inf
        m = e.max(axis=1, keepdims=True) if max_subtraction else np.zeros((e.shape[0], 1), dtype=e.dtype)
        p = np.exp(e - m)
        tot = p.sum(axis=1, keepdims=True, dtype=f)
        return (p / tot).astype(f)


def videos(lens):
    r0 = 0
    for T in lens:
        yield r0, int(T)
        r0 += int(T)


def alpha_spec(q, k, lens, scale, ignore_self=False, aperture=-1, dtype=np.float64, **softmax_kw):
    """[alpha (T, T) per video] in dtype."""
    out = []
    for r0, T in videos(lens):
        s = matmul(q[r0:r0 + T], np.asarray(k[r0:r0 + T]).T, dtype)
        out.append(softmax_rows(masked_logits(s, scale, ignore_self, aperture), **softmax_kw))
    return out


def keep_masks(lens, p, seed, local_rows=False):
    """[keep (T, T) bool per video]: element (packed row, key) -> dropout_keep(seed, 0, (row << 20) | key, p); everything kept at p == 0."""
    out = []
    for r0, T in videos(lens):
        if p <= 0.0:
            out.append(np.ones((T, T), dtype=bool))
            continue
        rows = np.arange(T, dtype=np.uint64) + np.uint64(0 if local_rows else r0)
        out.append(R.dropout_keep(seed, 0, (rows[:, None] << np.uint64(20)) | np.arange(T, dtype=np.uint64)[None, :], p))
    return out


def drop_scale(p):
    """fl32(1 / (1 - p)) as make_drop (csrc/sumk_internal.h) computes it."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0.0 else np.float32(1.0)


def dropped(x, keep, p, dtype):
    f = np.dtype(dtype).type
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.where(keep, np.asarray(x).astype(f) * f(drop_scale(p)), f(0.0)).astype(f)


def ds_spec(dctx, v, alpha, keep, p, scale, dtype=np.float64):
    """dS (T, T) of ONE video in dtype: scale * alpha * (d - sum_j d_j alpha_j), d = dropout'(dCTX V^T)."""
    f = np.dtype(dtype).type
    al = np.asarray(alpha).astype(f)
    d = dropped(matmul(dctx, np.asarray(v).T, dtype), keep, p, dtype)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dot = (d * al).sum(axis=1, keepdims=True, dtype=f)
        return (al * (d - dot) * f(np.float32(scale))).astype(f)


# ---------------------------------------------------------------------------------------------------------------- layouts
def ld_e(T):
    return (T + 3) & ~3


def ld_16(T):
    return (T + 63) & ~63


def sizes(lens):
    return sum(T * ld_e(T) for T in lens), sum(T * ld_16(T) for T in lens)


def split_e(flat, lens):
    """flat E buffer -> [(T, ldE) per video]"""
    out, o = [], 0
    for T in lens:
        out.append(np.asarray(flat[o:o + T * ld_e(T)]).reshape(T, ld_e(T)))
        o += T * ld_e(T)
    return out


def split_16(flat, lens):
    """flat P16 buffer (uint16 bit patterns) -> [(T, roundup64(T)) per video]"""
    out, o = [], 0
    for T in lens:
        out.append(np.asarray(flat[o:o + T * ld_16(T)]).reshape(T, ld_16(T)))
        o += T * ld_16(T)
    return out


# ---------------------------------------------------------------------------------------------------------------- the float32 model (+ mutants)
def _pad(a, width, dtype):
    out = np.zeros((a.shape[0], width), dtype=dtype)
    out[:, :a.shape[1]] = a
    return out


def model32_forward(c, mutant=None):
    """What the kernel writes, by the float32 specification: dict(E=[(T, ldE) float32], P16=[(T, ld16) uint16], O16=(rows, D) uint16)."""
    assert mutant is None or mutant in MUTANTS
    lens, p = c["lens"], c["p"]
    kw = {}
    if mutant == "no_max_subtraction":
        kw["max_subtraction"] = False
    al = []
    for n, (r0, T) in enumerate(videos(lens)):
        if mutant == "drop_last_key_tile":                    # the last 32-key tile of the LAST strip of every video left out of the softmax
            kw["drop_keys"] = (slice((T - 1) // 64 * 64, T), slice((T - 1) // 32 * 32, T)) if T > 32 else None
        al += alpha_spec(c["q"][r0:r0 + T], c["k"][r0:r0 + T], [T], c["scale"], c["ignore_self"], c["aperture"], np.float32, **kw)
    keep = keep_masks(lens, p, c["seed"], local_rows=mutant == "local_dropout_row")
    rnd = bf16_bits_trunc if mutant == "bf16_truncation" else bf16_bits
    E, P, O = [], [], np.zeros((sum(lens), c["D"]), dtype=np.uint16)
    for n, (r0, T) in enumerate(videos(lens)):
        E.append(_pad(al[n], ld_e(T), np.float32))
        pb = _pad(rnd(dropped(al[n], keep[n], p, np.float32)), ld_16(T), np.uint16)
        if mutant == "pad_column_nonzero" and ld_16(T) > T:
            pb[T // 2, T] = 0x3C00
        P.append(pb)
        pv = bf16_value(pb[:, :T])
        if mutant == "swap_p_chunks" and T >= 16:             # two 16-byte chunks (8 keys) of one row swapped before the second product
            row, a0, b0 = T // 2, 0, (T // 8 - 1) * 8
            pv = pv.copy()
            pv[row, a0:a0 + 8], pv[row, b0:b0 + 8] = pv[row, b0:b0 + 8].copy(), pv[row, a0:a0 + 8].copy()
        O[r0:r0 + T] = bf16_bits(matmul(pv, c["v"][r0:r0 + T], np.float32))
    return dict(E=E, P16=P, O16=O)


def model32_backward(c, E, mutant=None, keep=None):
    """The backward by the float32 specification, from the alpha blocks E ([(T, ldE)]): dict(P16=[(T, ld16) uint16 bf16(dS)], O16=(rows, D))."""
    lens, p = c["lens"], c["p"]
    keep = keep_masks(lens, p, c["seed"], local_rows=mutant == "local_dropout_row") if keep is None else keep
    rnd = bf16_bits_trunc if mutant == "bf16_truncation" else bf16_bits
    S, O = [], np.zeros((sum(lens), c["D"]), dtype=np.uint16)
    for n, (r0, T) in enumerate(videos(lens)):
        ds = ds_spec(c["dctx"][r0:r0 + T], c["v"][r0:r0 + T], E[n][:, :T], keep[n], p, c["scale"], np.float32)
        sb = _pad(rnd(ds), ld_16(T), np.uint16)
        S.append(sb)
        O[r0:r0 + T] = bf16_bits(matmul(bf16_value(sb[:, :T]), c["k"][r0:r0 + T], np.float32))
    return dict(P16=S, O16=O)


# ---------------------------------------------------------------------------------------------------------------- gates
class Gate:
    """Collects (got, float64 reference, float32 reference) triples of one family and one quantity; `check` then takes the yardstick -- the
    largest |float32 spec - float64 spec| over everything collected -- and asserts every element."""

    def __init__(self, what, half_bf16):
        self.what, self.half_bf16, self.items = what, half_bf16, []

    def add(self, tag, got, ref64, ref32):
        self.items.append((tag, np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64), np.asarray(ref32, dtype=np.float64)))

    def yardstick(self):
        y = 0.0
        with np.errstate(invalid="ignore"):
            for _, _, r64, r32 in self.items:
                d = np.abs(r32 - r64)
                d = d[~np.isnan(d)]
                if d.size:
                    y = max(y, float(d.max()))
        return y

    def check(self):
        """Returns (worst error / yardstick, yardstick).  Elements: |got - ref| <= 4 yardsticks + (bf16 quantities: half a bf16 spacing at
        max(|got|, |ref|); fp32 quantities: never less than 2 fp32 ulps of the reference).  NaN positions must agree; nothing is left out."""
        yard = self.yardstick()
        worst = 0.0
        for tag, got, r64, _ in self.items:
            assert np.array_equal(np.isnan(got), np.isnan(r64)), (self.what, tag, "NaN positions differ")
            ok = ~np.isnan(r64)
            g, r = got[ok], r64[ok]
            err = np.abs(g - r)
            if self.half_bf16:
                lim = bf16_half_spacing(np.maximum(np.abs(g), np.abs(r))) + MULT * yard
                excess = err - bf16_half_spacing(np.maximum(np.abs(g), np.abs(r)))
            else:
                lim = np.maximum(MULT * yard, 2.0 * np.spacing(np.abs(r).astype(np.float32)).astype(np.float64))
                excess = err
            bad = err > lim
            assert not bad.any(), (self.what, tag, "elements outside the gate", int(bad.sum()), "worst", float(err[bad].max()), "yardstick", yard)
            if err.size and yard > 0:
                worst = max(worst, float(max(excess.max(), 0.0) / yard))
        return worst, yard


def check_forward(fam, outs):
    """fam: cases; outs: per case dict(E, P16, O16) (model32_forward's layout, from the kernel or from a model).  Asserts the three forward
    stages on the family; returns {"E": (ratio, yardstick), "O16": (ratio, yardstick)}."""
    gE, gO = Gate("E", False), Gate("O16", True)
    for c, o in zip(fam, outs):
        lens, p = c["lens"], c["p"]
        a64 = alpha_spec(c["q"], c["k"], lens, c["scale"], c["ignore_self"], c["aperture"], np.float64)
        a32 = alpha_spec(c["q"], c["k"], lens, c["scale"], c["ignore_self"], c["aperture"], np.float32)
        keep = keep_masks(lens, p, c["seed"])
        for n, (r0, T) in enumerate(videos(lens)):
            tag = (c["name"], n, T)
            E, P = np.asarray(o["E"][n]), np.asarray(o["P16"][n])
            assert E.shape == (T, ld_e(T)) and P.shape == (T, ld_16(T)) and E.dtype == np.float32 and P.dtype == np.uint16, tag
            gE.add(tag, E[:, :T], a64[n], a32[n])
            assert not E[:, T:].view(np.uint32).any(), (tag, "E pad columns are not exactly 0")
            # P16: one fp32 multiply and one round to nearest even of the kernel's own E, bit for bit; NaN by position
            want = bf16_bits(dropped(E[:, :T], keep[n], p, np.float32))
            got = P[:, :T]
            gnan, wnan = np.isnan(bf16_value(got)), np.isnan(bf16_value(want))
            assert np.array_equal(gnan, wnan), (tag, "P16 NaN positions differ")
            neq = (got != want) & ~wnan
            assert not neq.any(), (tag, "P16 differs from bf16_rne(keep ? E * 1/(1-p) : 0)", int(neq.sum()), np.argwhere(neq)[:4].tolist())
            assert not P[:, T:].any(), (tag, "P16 pad columns are not exactly 0")
            pv = bf16_value(got)
            with np.errstate(invalid="ignore"):
                gO.add(tag, bf16_value(o["O16"][r0:r0 + T]), matmul(pv, c["v"][r0:r0 + T], np.float64), matmul(pv, c["v"][r0:r0 + T], np.float32))
    rE, yE = gE.check()
    # each finite row sums to 1 within the gate times T
    for tag, got, r64, _ in gE.items:
        fin = ~np.isnan(r64).any(axis=1)
        lim = max(MULT * yE, 2.0 * 2.0 ** -24) * tag[2]
        assert (np.abs(got[fin].sum(axis=1) - 1.0) <= lim).all(), (tag, "row sums", float(np.abs(got[fin].sum(axis=1) - 1.0).max()), lim)
    rO, yO = gO.check()
    return {"E": (rE, yE), "O16": (rO, yO)}


def check_backward(fam, Es, outs, keeps=None):
    """fam: cases (with dctx); Es: per case the alpha blocks the backward was given; outs: per case dict(P16, O16).  Asserts bf16(dS) against
    the float64 dS of those alphas and dQ against the product of the kernel's own bf16(dS).  keeps: per case keep masks to use instead of
    the specification's (the forward's mask read back from its P16)."""
    gS, gQ = Gate("dS", True), Gate("dQ", True)
    for ci, (c, E, o) in enumerate(zip(fam, Es, outs)):
        lens, p = c["lens"], c["p"]
        keep = keep_masks(lens, p, c["seed"]) if keeps is None else keeps[ci]
        for n, (r0, T) in enumerate(videos(lens)):
            tag = (c["name"], n, T)
            S = np.asarray(o["P16"][n])
            assert S.shape == (T, ld_16(T)) and S.dtype == np.uint16, tag
            al = np.asarray(E[n])[:, :T]
            args = (c["dctx"][r0:r0 + T], c["v"][r0:r0 + T], al, keep[n], p, c["scale"])
            gS.add(tag, bf16_value(S[:, :T]), ds_spec(*args, np.float64), ds_spec(*args, np.float32))
            # (0 as a VALUE: the kernel forms alpha * (d - dot) * scale with alpha = +0 there, which is -0 where d < dot)
            assert not (S[:, T:] & 0x7FFF).any(), (tag, "bf16(dS) pad columns are not 0")
            sv = bf16_value(S[:, :T])
            with np.errstate(invalid="ignore"):
                gQ.add(tag, bf16_value(o["O16"][r0:r0 + T]), matmul(sv, c["k"][r0:r0 + T], np.float64), matmul(sv, c["k"][r0:r0 + T], np.float32))
    rS, yS = gS.check()
    rQ, yQ = gQ.check()
    return {"dS": (rS, yS), "dQ": (rQ, yQ)}
