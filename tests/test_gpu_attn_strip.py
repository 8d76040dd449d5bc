"""GPU: the fused attention strips of the bf16 training step (csrc/attn_b16.hip, attn_strip_kernel<false / true>) through their own entry
(kernels.attn_strips_b16 / sumk_attn_strips_b16) against the float64 specification tests/attn_strip_ref.py, element by element and STAGE BY
STAGE, so that no stage's rounding is amplified by the next:

  forward   E    against the float64 alpha(Q, K): every element within 4 yardsticks (at least 2 fp32 ulps), the yardstick being the largest
                 |float32 spec - float64 spec| over the family; NaN positions equal; pad columns [T, ldE) exactly 0; finite rows sum to 1
            P16  BIT FOR BIT bf16_rne(keep ? E_got * fl32(1 / (1 - p)) : 0) of the kernel's own E; pad columns [T, roundup64(T)) exactly 0
            O16  against float64(P16_got) @ float64(V): |got - ref| <= half a bf16 spacing at max(|got|, |ref|) + 4 yardsticks
                 (yardstick: |float32 product - float64 product| of the same operands over the family)
  backward  P16  (bf16 dS) against the float64 dS of the E the forward wrote, and O16 (dQ) against float64(P16_got) @ float64(K), both under
                 the half-spacing + 4 yardsticks gate.
Nothing is left out of a comparison.  Every call runs with its three output buffers prefilled with 0xFF bytes inside 0xFF guard bands: after
the call the guards, and with ldo = 3 D the other 2 D columns, are untouched, and the backward leaves E as it was.

Families (tests/attn_strip_cases.py; tests/test_attn_strip_host.py proves on the CPU that these gates accept the float32 specification and
reject six deliberate mistakes): edges (one video, every NJ instance and every strip end), ragged batches of 1 .. 17 videos with dropout in
both operand layouts and both output widths, masks, width (D = 512, 1024, 2048), loud rows, dropout (four p, two seeds, the forward's mask
read back for the backward), determinism.  Every family prints its worst error / yardstick and keeps it in REPORT (written to
$SUMK_REPORT_DIR/attn_strip.json when set).
Measured on MI355X (2026-10-20), worst error / yardstick, E / O16 / dS / dQ (4 is the limit; for the three bf16 quantities the error beyond
half a bf16 spacing, which is why they are small: their error is almost all the one rounding to bf16): edges 0.53 / 0.06 / 0.01 / 0.08,
ragged 0.50 / 0.08 / 0.01 / 0.05, masks 0.91 / 0.05 / 0.01 / 0.07, width 0.65 / 0.02 / 0.00 / 0.01, loud 0.30 / 0.02 / 0.00 / 0.00,
dropout 0.57 / 0.03 / 0.01 / 0.01, the backward with the forward's mask read back 0.01 / 0.01.  E yardsticks: 1.0e-7 .. 2.4e-7 at D = 256,
2.9e-6 at D <= 2048, 3.6e-6 on the loud rows.  The kernel's v_exp_f32 needed no place in the float32 specification."""
import json
import os

import numpy as np
import pytest
import torch

import attn_strip_cases as cases
import attn_strip_ref as ref

pytestmark = pytest.mark.gpu
REPORT = {}
GUARD = 4096            # bytes of 0xFF on either side of every output buffer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "attn_strip.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


class Guarded:
    """nbytes of device memory filled with 0xFF between two guard bands of 0xFF."""

    def __init__(self, nbytes, dev):
        self.raw = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
        self.mid = self.raw[GUARD:GUARD + nbytes]
        assert self.mid.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xFF).all()) and bool((self.raw[GUARD + self.mid.numel():] == 0xFF).all())


def _b16(a, dev):
    return torch.from_numpy(a).to(dev).to(torch.bfloat16)           # the cases hold bf16 values: exact


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def call(c, dev, backward=False, layout="three", wide_out=False, E=None, seed=None):
    """One call of the entry on case c.  Forward: returns dict(E, P16, O16) in tests/attn_strip_ref.py's layout (+ E_dev for the backward).
    Backward: E is the device tensor the forward returned.  Asserts containment."""
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(c["lens"], dev)
    D, n = c["D"], sb.n_rows
    names = ("dctx", "v", "k") if backward else ("q", "k", "v")
    if layout == "three":
        a, b, cc = (_b16(c[m], dev) for m in names)
    else:                                                             # one [A | B | C] buffer, ld = 3 D
        buf = _b16(np.concatenate([c[m] for m in names], axis=1), dev)
        a, b, cc = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:]
    ne, np16 = kernels.attn_strips_b16_sizes(sb)
    assert (ne, np16) == ref.sizes(c["lens"])
    ldo = 3 * D if wide_out else D
    gO, gP = Guarded(n * ldo * 2, dev), Guarded(np16 * 2, dev)
    obuf = gO.mid.view(torch.bfloat16).view(n, ldo)
    out = obuf[:, D:2 * D] if wide_out else obuf                      # (the middle third: untouched columns on both sides)
    P = gP.mid.view(torch.bfloat16)
    if backward:
        gE, Et, e_before = None, E, E.clone()
    else:
        gE = Guarded(ne * 4, dev)
        Et = gE.mid.view(torch.float32)
    kernels.attn_strips_b16(backward, a, b, cc, out, Et, P, sb, c["scale"], ignore_self=c["ignore_self"], aperture=c["aperture"],
                            dropout_p=c["p"], seed=c["seed"] if seed is None else seed)
    torch.cuda.synchronize()
    assert gO.guards_intact() and gP.guards_intact() and (gE is None or gE.guards_intact()), (c["name"], "a guard band was written")
    if wide_out:
        ob = obuf.view(torch.int16)
        assert bool((ob[:, :D] == -1).all()) and bool((ob[:, 2 * D:] == -1).all()), (c["name"], "columns outside [D, 2 D) of the output rows were written")
    if backward:
        assert torch.equal(Et.view(torch.int32), e_before.view(torch.int32)), (c["name"], "the backward changed E")
    res = dict(P16=ref.split_16(_bits(P), c["lens"]), O16=_bits(out))
    if not backward:
        res["E"] = ref.split_e(Et.cpu().numpy(), c["lens"])
        res["E_dev"] = Et
    return res


def same_bits(x, y):
    return np.array_equal(x["O16"], y["O16"]) and all(np.array_equal(a, b) for a, b in zip(x["P16"], y["P16"])) and \
        all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x.get("E", []), y.get("E", [])))


def check_family(name, fam, dev, variants=(("three", False),)):
    outs, bwd = [], []
    for c in fam:
        o = call(c, dev, layout=variants[0][0], wide_out=variants[0][1])
        for lay, wide in variants[1:]:
            assert same_bits(o, call(c, dev, layout=lay, wide_out=wide)), (c["name"], lay, wide, "the layout changed the forward's bits")
        outs.append(o)
    r = ref.check_forward(fam, outs)
    both = [(c, o) for c, o in zip(fam, outs) if not c["forward_only"]]
    for c, o in both:
        s = call(c, dev, backward=True, layout=variants[0][0], wide_out=variants[0][1], E=o["E_dev"])
        for lay, wide in variants[1:]:
            assert same_bits(s, call(c, dev, backward=True, layout=lay, wide_out=wide, E=o["E_dev"])), (c["name"], lay, wide, "the layout changed the backward's bits")
        bwd.append(s)
    r.update(ref.check_backward([c for c, _ in both], [o["E"] for _, o in both], bwd))
    REPORT[name] = {k: dict(err_over_yardstick=v[0], yardstick=v[1]) for k, v in r.items()}
    REPORT[name]["cases"] = len(fam)
    print(f"attn_strip {name}: " + ", ".join(f"{k} {v[0]:.3f} yardsticks ({v[1]:.3e})" for k, v in r.items()) + f", {len(fam)} cases")
    return outs, bwd


def test_edges(dev):
    check_family("edges", cases.edges(), dev)


def test_ragged(dev):
    check_family("ragged", cases.ragged(), dev, variants=(("three", False), ("packed", False), ("three", True), ("packed", True)))


def test_masks(dev):
    outs, _ = check_family("masks", cases.masks(), dev)
    for c, o in zip(cases.masks(), outs):
        if c["lens"] == [1]:                    # ignore_self on a one-frame video: the row has no key left
            assert np.isnan(o["E"][0][:, :1]).all() and np.isnan(ref.bf16_value(o["P16"][0][:, :1])).all() and np.isnan(ref.bf16_value(o["O16"])).all()


def test_width(dev):
    check_family("width", cases.width(), dev)


def test_loud(dev):
    fam = cases.loud()
    outs, _ = check_family("loud", fam, dev)
    c, E = fam[0], outs[0]["E"]
    for r in c["saturating_rows"]:              # one weight exactly 1, every other exactly 0
        v, row = (0, r) if r < c["lens"][0] else (1, r - c["lens"][0])
        key = c["loud_keys"][v] - (c["lens"][0] if v else 0)
        assert E[v][row, key] == 1.0 and np.count_nonzero(E[v][row]) == 1, r


def test_dropout(dev):
    fam = cases.dropout()
    outs, _ = check_family("dropout", fam, dev)
    by = {c["name"]: (c, o) for c, o in zip(fam, outs)}
    (c11, o11), (c12, o12) = by["dropout_p0.5"], by["dropout_p0.5_seed12"]
    assert c11["seed"] != c12["seed"] and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(o11["E"], o12["E"]))
    assert any(not np.array_equal(a == 0, b == 0) for a, b in zip(o11["P16"], o12["P16"])), "two seeds gave one mask"
    # forward and backward of one seed use ONE mask: dS recomputed with the mask read back from the forward (P16 == 0 where E != 0)
    sel = [(c, o) for c, o in zip(fam, outs) if c["p"] > 0]
    keeps, bwd = [], []
    for c, o in sel:
        keeps.append([~((P[:, :T] == 0) & (E[:, :T] != 0)) for (_, T), E, P in zip(ref.videos(c["lens"]), o["E"], o["P16"])])
        dropped = 1.0 - np.mean(np.concatenate([k.ravel() for k in keeps[-1]]))
        assert abs(dropped - c["p"]) < 0.02, (c["name"], dropped)
        bwd.append(call(c, dev, backward=True, E=o["E_dev"]))
    r = ref.check_backward([c for c, _ in sel], [o["E"] for _, o in sel], bwd, keeps=keeps)
    REPORT["dropout_mask_read_back"] = {k: dict(err_over_yardstick=v[0], yardstick=v[1]) for k, v in r.items()}
    print("attn_strip dropout, mask read back: " + ", ".join(f"{k} {v[0]:.3f} yardsticks ({v[1]:.3e})" for k, v in r.items()))


def test_two_calls_are_bit_identical(dev):
    c = cases.ragged()[3]                       # 9 videos, dropout
    f1, f2 = call(c, dev, layout="packed", wide_out=True), call(c, dev, layout="packed", wide_out=True)
    assert same_bits(f1, f2)
    b1, b2 = (call(c, dev, backward=True, layout="packed", wide_out=True, E=f1["E_dev"]) for _ in range(2))
    assert same_bits(b1, b2)
