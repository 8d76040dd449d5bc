"""Numpy specification of the bf16x3 streaming attention (csrc/attn_stream_split.hip: kernels.attn_stream(..., precision="bf16x3")).
TEST INFRASTRUCTURE ONLY.

The dense formula of tests/attn_stream_ref.py (all logits of a row, the global row maximum) in float32 with the roundings of the bf16x3
arithmetic:
  * every operand x is two bf16 planes, hi = bf16(x) (round to nearest even) and lo = bf16(x - hi): oracle/torch_port.split_bf16;
  * a product is hi.hi + hi.lo + lo.hi, lo.lo dropped; each plane product is exact in float32, and they are added in ONE float32
    accumulator per output element walking k in ascending order (hi.hi, hi.lo, lo.hi at each k);
  * s = q3.k3; m = max_j s_j scale; p_j = exp(s_j scale - m) and tot = sum_j p_j in float32; the WEIGHTS p are split into two planes;
    O = p3.v3; ctx = O / tot; lse = m + log(tot).
This is the YARDSTICK of the GPU tests: what the arithmetic costs on a problem.  The REFERENCE stays attn_stream_ref.mha in float64 on the
unsplit inputs.  `acc=np.float64` sums the same plane products in float64 (tests/test_attn_stream_split_host.py holds that run to
oracle/torch_port.mm3).

`mutant` builds the wrong kernels the gate has to catch (tests/test_attn_stream_split_host.py):
  "first_no_lohi"   lo.hi dropped in the first product        "second_no_hilo"  hi.lo dropped in the second product
  "p_one_plane"     the weights as one bf16 plane             "natural_k"       V in natural key order under permuted weights: keys
  "drop_last_key"   the last key of a partial last tile lost                    16 g + 4 and 16 g + 8 swapped in the second product"""
import numpy as np

KEY_TILE = 64
MUTANTS = ("first_no_lohi", "second_no_hilo", "p_one_plane", "natural_k", "drop_last_key")


def bf16(x):
    """x (float32) rounded to the nearest bf16, ties to even, kept in float32; NaN stays NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = (u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    out = r.view(np.float32).copy()
    out[np.isnan(x)] = np.nan
    return out


def split(x):
    """(hi, lo) planes of a float32 array."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16(x)
    with np.errstate(invalid="ignore"):
        return hi, bf16(x - hi)


def chain3(a, b, acc=np.float32, terms=(True, True, True)):
    """a (M, K) @ b (K, N) in bf16x3: one accumulator of dtype `acc` per element, k ascending; terms: keep (hi.hi, hi.lo, lo.hi);
    a given as a (hi, lo) pair is taken as already split."""
    ah, al = a if isinstance(a, tuple) else split(a)
    bh, bl = split(b)
    f = np.dtype(acc).type
    ah, al, bh, bl = (t.astype(f) for t in (ah, al, bh, bl))
    out = np.zeros((ah.shape[0], bh.shape[1]), dtype=f)
    for k in range(ah.shape[1]):
        if terms[0]:
            out = out + ah[:, k, None] * bh[None, k, :]
        if terms[1]:
            out = out + ah[:, k, None] * bl[None, k, :]
        if terms[2]:
            out = out + al[:, k, None] * bh[None, k, :]
    return out


def mha3(Q, K, V, lens, n_heads, scale, acc=np.float32, mutant=None):
    """Q, K, V: (sum(lens), D) float32.  Returns (ctx (n, D), lse (n, n_heads)) in float32."""
    assert mutant is None or mutant in MUTANTS, mutant
    f = np.float32
    Q, K, V = (np.asarray(a, dtype=f) for a in (Q, K, V))
    n, D = Q.shape
    dh = D // n_heads
    sc = f(scale)
    ctx = np.zeros((n, D), dtype=f)
    lse = np.zeros((n, n_heads), dtype=f)
    r0 = 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for T in lens:
            rows = slice(r0, r0 + T)
            for h in range(n_heads):
                cols = slice(h * dh, (h + 1) * dh)
                q, k, v = Q[rows, cols], K[rows, cols], V[rows, cols]
                s = chain3(q, np.ascontiguousarray(k.T), acc, (True, True, mutant != "first_no_lohi")).astype(f)
                e = s * sc
                m = e.max(axis=1, keepdims=True)
                p = np.exp(e - m).astype(f)
                if mutant == "drop_last_key" and T % KEY_TILE:
                    p[:, T - 1] = 0
                tot = p.sum(axis=1, keepdims=True, dtype=f)
                ph, pl = split(p)
                if mutant == "p_one_plane":
                    pl = np.zeros_like(pl)
                vv = v
                if mutant == "natural_k":
                    vv = v.copy()
                    for g in range(0, T - 8, 16):
                        vv[[g + 4, g + 8]] = v[[g + 8, g + 4]]
                o = chain3((ph, pl), vv, acc, (True, mutant != "second_no_hilo", True)).astype(f)
                ctx[rows, cols] = o / tot
                lse[rows, h] = (m + np.log(tot))[:, 0]
            r0 += T
    return ctx, lse
