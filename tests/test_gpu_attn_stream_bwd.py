"""GPU: the training form of the streaming attention and its backward without the (T x T) blocks (csrc/attn_stream.hip: kernels.attn_stream_train;
csrc/attn_stream_bwd.hip: kernels.attn_stream_backward) against the float64 specification tests/attn_stream_bwd_ref.py, element by element of
ctx, dQ, dK and dV.

The gate is that of tests/test_gpu_attn_stream.py: the reference is the float64 specification, a family's yardstick per tensor is the largest
|float32 spec - float64 spec| over its cases, and every element must lie within max(4 yardsticks, 2 fp32 ulps of the value) of the reference;
NaN positions must agree exactly.  The float32 specification takes the dense route with one accumulator chain per product, so the
recomputation of the weights from the saved statistic, the regenerated masks and the two-pass order are what the yardstick does not contain.

Families (tests/attn_stream_bwd_cases.py): strips (one video, T at every edge of a wave block, a tile and a strip of both passes, head widths
4 .. 128, p = 0 and, at dh = 36 and 128, p = 0.1 and 0.5), ragged packed batches at p = 0.1 (and no leak across video boundaries), spikes
(late maxima, the staircase, underflow: the recomputed weights must agree with what the forward normalised by), the training forward (bits
of attn_stream at p = 0, the masks through one-hot V), determinism and graph capture, the in-place (R, 3 D) layouts, NaN rules, and buffers
past 2^31 bytes.  Every family prints its worst error / yardstick for ctx, dQ, dK, dV and keeps it in REPORT (written to
$SUMK_REPORT_DIR/attn_stream_bwd.json when set).
Measured on MI355X (2026-10-20), worst error / yardstick, ctx / dQ / dK / dV (4 is the limit): strips without dropout D16 h4 0.89 / 0.94 / 1.09 /
0.96, D32 h4 1.08 / 0.89 / 1.01 / 1.34, D72 h2 0.98 / 0.89 / 1.04 / 0.95, D200 h2 0.85 / 0.88 / 1.08 / 0.97, D128 h1 0.81 / 0.83 / 0.63 / 1.09,
D256 h2 1.03 / 1.00 / 1.15 / 0.90; with dropout D72 h2 p = 0.1 0.86 / 1.21 / 1.58 / 1.00, p = 0.5 0.96 / 0.62 / 1.01 / 0.88, D256 h2 p = 0.1
0.96 / 1.21 / 0.98 / 1.00, p = 0.5 0.98 / 1.25 / 1.14 / 1.04; ragged 1.21 / 1.07 / 1.11 / 0.80; spike 1.98 / 1.50 / 0.88 / 2.07; offsets
0.88 / 0.70 / 0.85 / 0.79; the finite elements of the NaN cases 1.28 / 0.73 / 1.03 / 1.14."""
import json
import os

import numpy as np
import pytest
import torch

import attn_stream_bwd_cases as cases
from attn_stream_bwd_ref import keep_mask, mha_train

pytestmark = pytest.mark.gpu
MULT = 4.0
TENSORS = ("ctx", "dq", "dk", "dv")
REPORT = {}


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
        with open(os.path.join(d, "attn_stream_bwd.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def bits(t):
    return t.contiguous().view(torch.int32)


def run(c, dev, layout="three", seed=cases.SEED):
    """{ctx, dq, dk, dv, stats} of a case through the two Python entries."""
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(c["lens"], dev)
    D = c["D"]
    g = torch.from_numpy(c["dctx"]).to(dev)
    if layout == "three":
        q, k, v = (torch.from_numpy(c[n]).to(dev) for n in "qkv")
    else:
        buf = torch.from_numpy(np.concatenate([c["q"], c["k"], c["v"]], axis=1)).to(dev)
        q, k, v = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:]
    kw = dict(scale=c["scale"], dropout_p=c["p"], seed=seed, site=cases.SITE)
    ctx, stats = kernels.attn_stream_train(q, k, v, sb, c["heads"], **kw)
    dq, dk, dv = kernels.attn_stream_backward(q, k, v, ctx, g, stats, sb, c["heads"], **kw)
    return dict(ctx=ctx, dq=dq, dk=dk, dv=dv, stats=stats)


def worst(got, ref64, yard, what):
    """max over elements of |got - ref| / yardstick after asserting every element inside max(4 yardsticks, 2 ulps)."""
    got = got.double().cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), (what, "NaN positions differ", int(np.isnan(got).sum()), int(np.isnan(ref64).sum()))
    ok = ~np.isnan(ref64)
    err = np.abs(got[ok] - ref64[ok])
    gate = np.maximum(MULT * yard, 2.0 * np.spacing(np.abs(ref64[ok]).astype(np.float32)).astype(np.float64))
    bad = err > gate
    assert not bad.any(), (what, float(err.max()), yard, int(bad.sum()))
    return float(err.max() / yard) if yard > 0 and err.size else 0.0


def yardsticks(fam):
    with np.errstate(invalid="ignore"):
        return {t: max(float(np.nanmax(np.abs(cases.spec(c)[1][t] - cases.spec(c)[0][t]))) for c in fam) for t in TENSORS}


def check_family(name, fam, dev, layouts=("three",)):
    yard = yardsticks(fam)
    ratio = dict.fromkeys(TENSORS, 0.0)
    for c in fam:
        s64 = cases.spec(c)[0]
        for lay in layouts:
            got = run(c, dev, lay)
            for t in TENSORS:
                ratio[t] = max(ratio[t], worst(got[t], s64[t], yard[t], (c["name"], lay, t)))
    REPORT[name] = dict(err_over_yardstick=ratio, yardstick=yard, cases=len(fam))
    print(f"attn_stream_bwd {name}: " + ", ".join(f"{t} {ratio[t]:.3f} yardsticks ({yard[t]:.3e})" for t in TENSORS) + f", {len(fam)} cases")
    return ratio


@pytest.mark.parametrize("D,heads", cases.STRIP_SHAPES)
def test_strips(dev, D, heads):
    check_family(f"strips_D{D}_h{heads}_p0.0", cases.strips(D, heads, 0.0), dev, layouts=("three", "packed"))


@pytest.mark.parametrize("D,heads", cases.STRIP_DROPOUT)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_strips_with_dropout(dev, D, heads, p):
    check_family(f"strips_D{D}_h{heads}_p{p}", cases.strips(D, heads, p), dev)


def test_ragged_and_no_leak_across_videos(dev):
    fam = cases.ragged()
    check_family("ragged", fam, dev, layouts=("three", "packed"))
    c = fam[0]                                                # lens (1, 64, 65, 200, 3, 129), D = 256
    base = run(c, dev)
    lo, hi = 1 + 64, 1 + 64 + 65                              # perturb video 2 alone: every input, every row
    d = dict(c)
    for n in ("q", "k", "v", "dctx"):
        d[n] = c[n].copy()
        d[n][lo:hi] = d[n][lo:hi] * 1.5 + 0.25
    got = run(d, dev)
    for t in TENSORS:
        assert torch.equal(bits(got[t][:lo]), bits(base[t][:lo])) and torch.equal(bits(got[t][hi:]), bits(base[t][hi:])), (t, "leaked")
        assert not torch.equal(bits(got[t][lo:hi]), bits(base[t][lo:hi])), t


def test_spike(dev):
    check_family("spike", cases.spikes(), dev)


def test_training_forward(dev):
    """ctx at p = 0.1 and 0.5 is gated with the strips; here: p = 0 gives attn_stream's bits, and the masks are recipes.dropout_keep's."""
    from summarizer_amd import kernels
    for c0 in (cases.fwd.case("fwd", (1, 64, 65, 200, 3, 129), 256, 2, 21), cases.fwd.case("fwd36", (129, 70), 72, 2, 22)):
        sb = kernels.SeqBatch.get(c0["lens"], dev)
        q, k, v = (torch.from_numpy(c0[n]).to(dev) for n in "qkv")
        plain = kernels.attn_stream(q, k, v, sb, c0["heads"])
        ctx, stats = kernels.attn_stream_train(q, k, v, sb, c0["heads"], dropout_p=0.0, seed=5, site=3)
        assert torch.equal(bits(ctx), bits(plain)), "p = 0 changed the bits of ctx"
        _, lse = kernels.attn_stream(q, k, v, sb, c0["heads"], want_lse=True)
        got = stats[:, :, 0].double() + torch.log(stats[:, :, 1].double())
        assert float((got - lse.double()).abs().max()) <= 1e-5 * float(lse.abs().max())
    # one-hot V at T = 65, dh = 4: 17 heads, V = the 65 x 68 identity, so head j // 4 sees key j alone in its column j % 4 and, with Q = 0
    # (alpha = 1 / T), ctx[i, j] = keep(i, head j // 4, key j) ? 1 / (T (1 - p)) : 0 -- every mask bit of those (row, head, key) by itself
    T, heads = 65, 17
    D, lead = 4 * heads, 3
    sb = kernels.SeqBatch.get([lead, T], dev)                 # a first video, so that packed rows differ from rows
    v = np.zeros((lead + T, D), dtype=np.float32)
    v[lead + np.arange(T), np.arange(T)] = 1.0
    z = torch.zeros(lead + T, D, device=dev)
    for p in (0.1, 0.5):
        ctx, _ = kernels.attn_stream_train(z, z, torch.from_numpy(v).to(dev), sb, heads, dropout_p=p, seed=cases.SEED, site=cases.SITE)
        ctx = ctx.cpu().numpy()[lead:]
        keep = np.stack([keep_mask(cases.SEED, cases.SITE, p, lead, T, heads, j // 4)[:, j] for j in range(T)], axis=1)
        assert 0.3 * p < 1.0 - keep.mean() < 2.0 * p
        assert np.array_equal(ctx[:, :T] != 0, keep), (p, "kept entries differ from recipes.dropout_keep")
        want = 1.0 / T / (1.0 - float(np.float32(p)))
        assert np.abs(ctx[:, :T][keep] - want).max() <= 4 * np.spacing(np.float32(want)) and not ctx[:, T:].any()


def test_training_forward_head_width_256_with_dropout(dev):
    """The one training-forward instance no other test launches: head width 256 (as_stream_kernel<8, true>, 130 KiB of dynamic LDS, which the
    backward refuses).  ctx against the float64 specification by the family's rule: yardstick |float32 spec - float64 spec|, limit 4.  T = 129 and
    65: two strips, a partial last tile, waves past the video, a second video behind the first."""
    from summarizer_amd import kernels
    c = cases.with_grad(cases.fwd.case("fwd256", (129, 65), 256, 1, 23), 0.1)
    s64, s32 = cases.spec(c)
    yard = float(np.abs(s32["ctx"] - s64["ctx"]).max())
    sb = kernels.SeqBatch.get(c["lens"], dev)
    q, k, v = (torch.from_numpy(c[n]).to(dev) for n in "qkv")
    ctx, stats = kernels.attn_stream_train(q, k, v, sb, 1, dropout_p=c["p"], seed=cases.SEED, site=cases.SITE)
    r = worst(ctx, s64["ctx"], yard, (c["name"], "ctx"))
    print(f"attn_stream_train dh 256, p 0.1: ctx {r:.3f} yardsticks ({yard:.3e})")
    assert bool(torch.isfinite(stats).all())


def test_determinism_and_capture(dev):
    from summarizer_amd import kernels
    c = cases.with_grad(cases.fwd.case("det", (1, 64, 65, 200, 3, 129), 256, 2, 21), 0.1)
    a, b = run(c, dev), run(c, dev)
    for t in TENSORS + ("stats",):
        assert torch.equal(bits(a[t]), bits(b[t])), t
    other = run(c, dev, seed=cases.SEED + 1)
    assert not torch.equal(bits(other["dq"]), bits(a["dq"])), "another seed drew the same masks"
    sb = kernels.SeqBatch.get(c["lens"], dev)
    q, k, v, g = (torch.from_numpy(c[n]).to(dev) for n in ("q", "k", "v", "dctx"))
    kw = dict(dropout_p=0.1, seed=cases.SEED, site=cases.SITE)

    def step():
        ctx, stats = kernels.attn_stream_train(q, k, v, sb, 2, **kw)
        return (ctx,) + kernels.attn_stream_backward(q, k, v, ctx, g, stats, sb, 2, **kw)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    c2 = cases.with_grad(cases.fwd.case("det2", c["lens"], 256, 2, 22), 0.1)
    for dst, n in ((q, "q"), (k, "k"), (v, "v"), (g, "dctx")):
        dst.copy_(torch.from_numpy(c2[n]))
    graph.replay()
    torch.cuda.synchronize()
    want = run(c2, dev)
    for o, t in zip(outs, TENSORS):
        assert torch.equal(bits(o), bits(want[t])), (t, "replay differs")
        assert not torch.equal(bits(o), bits(a[t])), t


def test_in_place_layouts(dev):
    """Q | K | V in one (R, 3 D) buffer and dQ | dK | dV in another, ld = 3 D, through the raw entry; the result has the bits of three buffers."""
    from summarizer_amd import _lib, kernels
    lib = _lib.load()
    c = cases.with_grad(cases.fwd.case("inplace", (65, 130, 7), 200, 2, 33), 0.1)       # dh = 100: scale = 0.1
    want = run(c, dev)
    D, R = c["D"], sum(c["lens"])
    sb = kernels.SeqBatch.get(c["lens"], dev)
    buf = torch.from_numpy(np.concatenate([c["q"], c["k"], c["v"]], axis=1)).to(dev)
    out = torch.full((R, 3 * D), float("nan"), device=dev)
    g = torch.from_numpy(c["dctx"]).to(dev)
    nb = kernels.attn_stream_backward_workspace_bytes(D, 2, sb)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    p = lambda t, col=0: t.data_ptr() + 4 * col
    rc = lib.sumk_attn_stream_backward(p(buf), 3 * D, p(buf, D), 3 * D, p(buf, 2 * D), 3 * D, p(want["ctx"]), D, p(g), D, p(want["stats"]), D, 2,
                                       sb.n_seq, sb.off_host_p, sb.off_dev_p, 0.1, 0.1, cases.SEED, cases.SITE, p(out), 3 * D, p(out, D), 3 * D,
                                       p(out, 2 * D), 3 * D, p(ws), nb, kernels._stream())
    assert rc == 0, lib.sumk_last_error()
    for i, t in enumerate(("dq", "dk", "dv")):
        assert torch.equal(bits(out[:, i * D:(i + 1) * D]), bits(want[t])), t


def test_nan_rules(dev):
    """A NaN in one K row, one Q row, one dctx row: NaN positions as the float64 specification has them, the finite elements inside the gate
    (yardstick: the float32 specification on the same inputs), nothing outside the video."""
    c = cases.with_grad(cases.fwd.case("nan", (70, 130, 40), 64, 2, 11), 0.1)
    base = run(c, dev)
    fam = []
    for which, row in (("k", 150), ("q", 100), ("dctx", 199)):
        d = dict(c, name=f"nan_{which}_{row}", **{which: c[which].copy()})
        d[which][row, 40] = np.nan                            # head 1
        fam.append(d)
    yard = yardsticks(fam)
    ratio = dict.fromkeys(TENSORS, 0.0)
    for d in fam:
        s64, s32 = cases.spec(d)
        got = run(d, dev)
        for t in TENSORS:
            assert np.array_equal(np.isnan(s32[t]), np.isnan(s64[t])), (d["name"], t)
            ratio[t] = max(ratio[t], worst(got[t], s64[t], yard[t], (d["name"], t)))
            assert np.isnan(s64[t][70:200]).any() or t == "ctx", (d["name"], t)
            for lo, hi in ((0, 70), (200, 240)):              # the other videos: not a bit
                assert torch.equal(bits(got[t][lo:hi]), bits(base[t][lo:hi])), (d["name"], t)
            assert not bool(torch.isnan(got[t][:, :32]).any()), (d["name"], t, "NaN crossed into head 0")
    REPORT["nan"] = dict(err_over_yardstick=ratio, yardstick=yard, cases=len(fam))
    print("attn_stream_bwd nan: " + ", ".join(f"{t} {ratio[t]:.3f} yardsticks ({yard[t]:.3e})" for t in TENSORS))


def test_offsets_past_2_31_bytes(dev):
    """704 videos of 256 frames at D = 1024 in the (R, 3 D) layout: both buffers are 2.2e9 bytes, so the last videos lie past 2^31 bytes."""
    from summarizer_amd import kernels
    n_vid, T, D, heads = 704, 256, 1024, 8
    rows = n_vid * T
    assert rows * 3 * D * 4 > 2 ** 31
    need = 2 * rows * 3 * D * 4 + 3 * rows * D * 4 + (1 << 28)
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"the device has {free} bytes free, the buffers need {need}")
    gen = torch.Generator(device=dev).manual_seed(5)
    buf = torch.randn(rows, 3 * D, device=dev, generator=gen)
    g = torch.randn(rows, D, device=dev, generator=gen)
    out = torch.empty(rows, 3 * D, device=dev)
    sb = kernels.SeqBatch.get([T] * n_vid, dev)
    kw = dict(dropout_p=0.1, seed=cases.SEED, site=cases.SITE)
    q, k, v = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:]
    ctx, stats = kernels.attn_stream_train(q, k, v, sb, heads, **kw)
    dq, dk, dv = kernels.attn_stream_backward(q, k, v, ctx, g, stats, sb, heads, out=out, **kw)
    n = 3 * T
    tail, gt = buf[-n:].cpu().numpy(), g[-n:].cpu().numpy()
    # the specification on the last three videos alone; their masks are indexed by the packed row
    a = (tail[:, :D], tail[:, D:2 * D], tail[:, 2 * D:], gt, [T] * 3, heads, 1.0 / np.sqrt(D // heads), 0.1, cases.SEED, cases.SITE)
    s64, s32 = mha_train(*a, row0=rows - n), mha_train(*a, dtype=np.float32, row0=rows - n)
    ratio = {}
    for t, got in (("ctx", ctx), ("dq", dq), ("dk", dk), ("dv", dv)):
        ratio[t] = worst(got[-n:], s64[t], float(np.abs(s32[t] - s64[t]).max()), ("offsets", t))
    REPORT["offsets"] = dict(err_over_yardstick=ratio)
    print("attn_stream_bwd offsets: " + ", ".join(f"{t} {ratio[t]:.3f} yardsticks" for t in TENSORS))
    del buf, g, out, ctx, stats, dq, dk, dv
    torch.cuda.empty_cache()
