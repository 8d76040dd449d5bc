"""GPU: multi-head attention without the (T x T) logits (csrc/attn_stream.hip: kernels.attn_stream / sumk_attn_stream) against the float64
specification tests/attn_stream_ref.py, element by element of ctx and of lse.

The project's gate: the reference is the float64 specification, a family's yardstick is the largest |float32 spec - float64 spec| over its
cases (ctx and lse apart), and every element must lie within 4 yardsticks (at least 2 fp32 ulps of the value) of the reference.  Nothing is
left out of a comparison; NaN positions must agree exactly.  The float32 specification sums both products as one accumulator chain in the
DENSE order, so the kernel's online rescale is the one thing the yardstick does not contain.

Families (tests/attn_stream_cases.py): strips (one video, T at every edge of a 32-row wave block, a 64-key tile and a 128-row strip, head
widths 4 .. 256, both operand layouts), ragged packed batches with loud edge frames, spikes that force the rescale (a late maximum of +20,
+60, +120 at four key positions, a staircase, weights underflowing to 0), NaN rules, determinism / poisoned scratch / graph capture, a
[Q | K | V] buffer past 2^31 bytes, and the raw entry's refusals.  Every family prints its worst error / yardstick and keeps it in REPORT
(written to $SUMK_REPORT_DIR/attn_stream.json when set).
Measured on MI355X (2026-10-20), worst error / yardstick, ctx / lse (4 is the limit): strips D16 h4 0.89 / 1.00, D32 h4 1.08 / 0.76, D72 h2
0.98 / 0.99, D200 h2 0.85 / 1.00, D128 h1 0.81 / 1.20, D256 h2 1.03 / 0.98, D512 h2 1.19 / 0.82; ragged 1.17 / 0.91; spike 1.98 / 1.00;
offsets 0.95 / 1.27; the finite elements of the NaN cases 0.70 / 1.10."""
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_stream_cases as cases
from attn_stream_ref import mha

pytestmark = pytest.mark.gpu
MULT = 4.0
REPORT = {}
_SPEC = {}


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
        with open(os.path.join(d, "attn_stream.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def spec(c):
    """(ctx64, lse64, ctx32, lse32) of a case, computed once."""
    if c["name"] not in _SPEC:
        sc = cases.scale_of(c)
        _SPEC[c["name"]] = mha(c["q"], c["k"], c["v"], c["lens"], c["heads"], sc) + mha(c["q"], c["k"], c["v"], c["lens"], c["heads"], sc, np.float32)
    return _SPEC[c["name"]]


def run(c, dev, layout="three", want_lse=True):
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(c["lens"], dev)
    D = c["D"]
    if layout == "three":
        q, k, v = (torch.from_numpy(c[n]).to(dev) for n in "qkv")
    else:
        buf = torch.from_numpy(np.concatenate([c["q"], c["k"], c["v"]], axis=1)).to(dev)
        q, k, v = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:]
    return kernels.attn_stream(q, k, v, sb, c["heads"], scale=c["scale"], want_lse=want_lse)


def worst(got, ref64, yard, what):
    """max over elements of |got - ref| / yardstick after asserting every element inside max(4 yardsticks, 2 ulps)."""
    got = got.double().cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), (what, "NaN positions differ")
    ok = ~np.isnan(ref64)
    err = np.abs(got[ok] - ref64[ok])
    gate = np.maximum(MULT * yard, 2.0 * np.spacing(np.abs(ref64[ok]).astype(np.float32)).astype(np.float64))
    bad = err > gate
    assert not bad.any(), (what, float(err.max()), yard, int(bad.sum()))
    return float(err.max() / yard) if yard > 0 else 0.0


def check_family(name, fam, dev, layouts=("three",)):
    yc = max(float(np.abs(spec(c)[2] - spec(c)[0]).max()) for c in fam)
    yl = max(float(np.abs(spec(c)[3] - spec(c)[1]).max()) for c in fam)
    rc = rl = 0.0
    for c in fam:
        c64, l64 = spec(c)[:2]
        for lay in layouts:
            ctx, lse = run(c, dev, lay)
            rc = max(rc, worst(ctx, c64, yc, (c["name"], lay, "ctx")))
            rl = max(rl, worst(lse, l64, yl, (c["name"], lay, "lse")))
            ctx2 = run(c, dev, lay, want_lse=False)
            assert torch.equal(ctx.view(torch.int32), ctx2.view(torch.int32)), (c["name"], lay, "want_lse changed ctx")
    REPORT[name] = dict(ctx_err_over_yardstick=rc, lse_err_over_yardstick=rl, ctx_yardstick=yc, lse_yardstick=yl, cases=len(fam))
    print(f"attn_stream {name}: ctx {rc:.3f} yardsticks ({yc:.3e}), lse {rl:.3f} yardsticks ({yl:.3e}), {len(fam)} cases")


@pytest.mark.parametrize("D,heads", cases.STRIP_SHAPES)
def test_strips(dev, D, heads):
    check_family(f"strips_D{D}_h{heads}", cases.strips(D, heads), dev, layouts=("three", "packed"))


def test_ragged(dev):
    check_family("ragged", cases.ragged(), dev, layouts=("three", "packed"))


def test_spike(dev):
    check_family("spike", cases.spikes(), dev)


def test_nan_rules(dev):
    """NaN positions as the float64 specification has them, the other videos bit-equal to the run without NaN, and every finite element
    -- those of the poisoned video included -- inside the family's gate (yardstick: the float32 specification on the same four inputs)."""
    c = cases.case("nan", (70, 130, 40), 64, 2, 11)
    base, base_lse = run(c, dev)
    fam = []
    for which, row, col in (("q", 100, None), ("k", 150, 40), ("v", 199, None), ("v", 71, 5)):
        d = dict(c, name=f"nan_{which}_{row}_{col}", **{which: c[which].copy()})
        if col is None:
            d[which][row] = np.nan
        else:
            d[which][row, col] = np.nan
        fam.append(d)
    with np.errstate(invalid="ignore"):
        yc = max(float(np.nanmax(np.abs(spec(d)[2] - spec(d)[0]))) for d in fam)
        yl = max(float(np.nanmax(np.abs(spec(d)[3] - spec(d)[1]))) for d in fam)
    rc = rl = 0.0
    out = {}
    for d in fam:
        got, lse = run(d, dev)
        assert np.array_equal(np.isnan(spec(d)[2]), np.isnan(spec(d)[0])) and np.array_equal(np.isnan(spec(d)[3]), np.isnan(spec(d)[1])), d["name"]
        rc = max(rc, worst(got, spec(d)[0], yc, (d["name"], "ctx")))          # NaN positions equal, every finite element gated
        rl = max(rl, worst(lse, spec(d)[1], yl, (d["name"], "lse")))
        for lo, hi in ((0, 70), (200, 240)):              # the other videos: not a bit
            assert torch.equal(got[lo:hi].view(torch.int32), base[lo:hi].view(torch.int32)), d["name"]
            assert torch.equal(lse[lo:hi].view(torch.int32), base_lse[lo:hi].view(torch.int32)), d["name"]
        out[d["name"]] = (got.cpu().numpy(), lse.cpu().numpy())
    REPORT["nan"] = dict(ctx_err_over_yardstick=rc, lse_err_over_yardstick=rl, ctx_yardstick=yc, lse_yardstick=yl, cases=len(fam))
    print(f"attn_stream nan: ctx {rc:.3f} yardsticks ({yc:.3e}), lse {rl:.3f} yardsticks ({yl:.3e}), {len(fam)} cases")
    g, l = out["nan_q_100_None"]
    assert np.isnan(g[100]).all() and not np.isnan(np.delete(g, 100, 0)).any() and np.isnan(l[100]).all() and np.isnan(l).sum() == 2
    g, l = out["nan_k_150_40"]
    assert np.isnan(g[70:200, 32:]).all() and not np.isnan(g[70:200, :32]).any() and np.isnan(l[70:200, 1]).all() and np.isnan(l).sum() == 130
    g, l = out["nan_v_199_None"]
    assert np.isnan(g[70:200]).all() and not np.isnan(l).any()
    g, l = out["nan_v_71_5"]
    assert np.isnan(g[70:200, 5]).all() and np.isnan(g).sum() == 130 and not np.isnan(l).any()


def test_determinism_scratch_and_capture(dev):
    from summarizer_amd import kernels
    c = cases.case("det", (1, 64, 65, 200, 3, 129), 256, 2, 21)
    sb = kernels.SeqBatch.get(c["lens"], dev)
    q, k, v = (torch.from_numpy(c[n]).to(dev) for n in "qkv")
    bits = lambda t: t.view(torch.int32)
    a, la = kernels.attn_stream(q, k, v, sb, 2, want_lse=True)
    b, lb = kernels.attn_stream(q, k, v, sb, 2, want_lse=True)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(la), bits(lb))
    # workspace and outputs pre-filled with 0xFF bytes, through the raw entry
    lib = __import__("summarizer_amd._lib", fromlist=["load"]).load()
    nb = kernels.attn_stream_workspace_bytes(256, 2, sb)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    ctx = torch.full((sb.n_rows, 256), float("nan"), device=dev); ctx.view(torch.int32).fill_(-1)
    lse = torch.empty(sb.n_rows, 2, device=dev); lse.view(torch.int32).fill_(-1)
    rc = lib.sumk_attn_stream(q.data_ptr(), 256, k.data_ptr(), 256, v.data_ptr(), 256, 256, 2, sb.n_seq, sb.off_host_p, sb.off_dev_p,
                              1.0 / math.sqrt(128), ctx.data_ptr(), 256, lse.data_ptr(), ws.data_ptr(), nb, kernels._stream())
    assert rc == 0, lib.sumk_last_error()
    assert torch.equal(bits(ctx), bits(a)) and torch.equal(bits(lse), bits(la))
    # one call captured into a graph, replayed twice on changed inputs
    qs, ks, vs = q.clone(), k.clone(), v.clone()
    kernels.attn_stream(qs, ks, vs, sb, 2, want_lse=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gc, gl = kernels.attn_stream(qs, ks, vs, sb, 2, want_lse=True)
    for seed in (22, 23):
        c2 = cases.case("det2", c["lens"], 256, 2, seed)
        for dst, n in ((qs, "q"), (ks, "k"), (vs, "v")):
            dst.copy_(torch.from_numpy(c2[n]))
        graph.replay()
        torch.cuda.synchronize()
        e, le = kernels.attn_stream(qs, ks, vs, sb, 2, want_lse=True)
        assert torch.equal(bits(gc), bits(e)) and torch.equal(bits(gl), bits(le)), seed
        assert not torch.equal(bits(e), bits(a))


def test_offsets_past_2_31_bytes(dev):
    """2800 videos of 64 frames at D = 1024: the (rows, 3 D) buffer is 2.2e9 bytes, so the last videos' offsets do not fit 31 bits."""
    from summarizer_amd import kernels
    n_vid, T, D, heads = 2800, 64, 1024, 8
    rows = n_vid * T
    assert rows > 174763 and rows * 3 * D * 4 > 2 ** 31
    g = torch.Generator(device=dev).manual_seed(5)
    buf = torch.randn(rows, 3 * D, device=dev, generator=g)
    sb = kernels.SeqBatch.get([T] * n_vid, dev)
    ctx, lse = kernels.attn_stream(buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:], sb, heads, want_lse=True)
    tail = buf[-3 * T:].cpu().numpy()
    c = dict(name="offsets_tail", lens=[T] * 3, D=D, heads=heads, scale=None, q=tail[:, :D], k=tail[:, D:2 * D], v=tail[:, 2 * D:])
    c64, l64, c32, l32 = spec(c)
    rc = worst(ctx[-3 * T:], c64, float(np.abs(c32 - c64).max()), "offsets ctx")
    rl = worst(lse[-3 * T:], l64, float(np.abs(l32 - l64).max()), "offsets lse")
    REPORT["offsets"] = dict(ctx_err_over_yardstick=rc, lse_err_over_yardstick=rl)
    print(f"attn_stream offsets: ctx {rc:.3f} yardsticks, lse {rl:.3f} yardsticks")
    del buf, ctx, lse
    torch.cuda.empty_cache()


def test_raw_entry_refusals(dev):
    from summarizer_amd import _lib, kernels
    lib = _lib.load()
    PAT = 0x5A5A5A5A

    def call(D, heads, lens, ld=None, ctx_null=False, short=0, want=-1, msg=b"", scale=0.25):
        ld = D if ld is None else ld
        rows = max(sum(lens), 1)
        off_host = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        off_dev = torch.from_numpy(off_host).to(dev)
        q = torch.zeros(rows, max(ld, D), device=dev)
        ctx = torch.empty(rows, max(ld, D), device=dev); ctx.view(torch.int32).fill_(PAT)
        lse = torch.empty(rows, heads, device=dev); lse.view(torch.int32).fill_(PAT)
        nb = max(int(lib.sumk_attn_stream_workspace_bytes(D, heads, len(lens), _lib.host_i32(off_host))), 256)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev); ws.fill_(0x5A)
        rc = lib.sumk_attn_stream(q.data_ptr(), ld, q.data_ptr(), ld, q.data_ptr(), ld, D, heads, len(lens), _lib.host_i32(off_host),
                                  off_dev.data_ptr(), scale, None if ctx_null else ctx.data_ptr(), ld, lse.data_ptr(), ws.data_ptr(),
                                  nb - short, kernels._stream())
        torch.cuda.synchronize()
        assert rc == want, (rc, want, lib.sumk_last_error())
        if want != 0:
            assert msg in lib.sumk_last_error(), (msg, lib.sumk_last_error())
            assert bool((ctx.view(torch.int32) == PAT).all()) and bool((lse.view(torch.int32) == PAT).all()), msg
            assert bool((ws == 0x5A).all()), msg
    call(64, 2, [10], want=0)
    call(520, 2, [10], msg=b"head width 260")
    call(12, 2, [10], msg=b"head width 6")
    call(64, 2, [10], ld=60, msg=b"must be at least D=64")
    call(64, 2, [10], ld=66, msg=b"multiples of 4")
    call(64, 2, [10], ctx_null=True, msg=b"null pointer")
    call(64, 2, [10, 0, 5], msg=b"video 1 has 0 frames")
    call(64, 2, [10], short=1, want=-2, msg=b"workspace 255 < required 256")
    for bad in (0.0, -0.125, float("inf"), float("nan")):     # the row maximum is taken before scaling: the scale must be positive and finite
        call(64, 2, [10], scale=bad, msg=b"must be positive and finite")
