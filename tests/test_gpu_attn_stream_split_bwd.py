"""GPU: the training form of the streaming attention and its backward in bf16x3 (csrc/attn_stream_split.hip: kernels.attn_stream_train(...,
precision="bf16x3"); csrc/attn_stream_split_bwd.hip: kernels.attn_stream_backward(..., precision="bf16x3")) against the float64
specification tests/attn_stream_bwd_ref.mha_train on the unsplit inputs, element by element of ctx, dQ, dK and dV.

The gate is that of tests/test_gpu_attn_stream_split.py: a family's yardstick per tensor is the largest |bf16x3 specification - float64
specification| over its cases (tests/attn_stream_split_bwd_ref.py: what the arithmetic costs), and every element must lie within 4
yardsticks (at least 2 fp32 ulps of the value) of the float64 reference.  Nothing is left out of a comparison; NaN positions must agree
exactly.  tests/test_attn_stream_split_bwd_host.py shows that the yardsticks are not blown up (at most 4 x 2^8 fp32 yardsticks) and that
the gate catches seven wrong kernels.

Families (tests/attn_stream_split_bwd_cases.py): strips at head widths 8, 40, 104, 128 in both operand layouts, with dropout at 40 and 128,
ragged batches, spikes; exact small-integer data (the lane maps and the transposed operands, to the bit), the masks bit by bit, p = 0
against the scoring call, determinism / poisoned workspace / graph capture, NaN rules, buffers and planes past 2^31 bytes, and the
untouched fp32 calls.  Every family prints its worst error / yardstick for ctx, dQ, dK, dV and keeps it in REPORT
($SUMK_REPORT_DIR/attn_stream_split_bwd.json when set).
Measured on MI355X (2026-10-21), worst error / yardstick, ctx / dQ / dK / dV (4 is the limit): strips without dropout D32 h4 0.97 / 1.00 / 1.05 /
0.94, D80 h2 1.00 / 1.03 / 1.02 / 1.03, D208 h2 0.93 / 1.05 / 1.12 / 0.98, D128 h1 1.16 / 1.00 / 0.98 / 1.11, D256 h2 1.05 / 1.00 / 1.02 / 0.93; with
dropout D80 h2 p = 0.1 1.00 / 0.99 / 1.05 / 0.96, p = 0.5 0.99 / 1.00 / 0.98 / 1.00, D256 h2 p = 0.1 1.03 / 1.04 / 0.93 / 1.03, p = 0.5 1.07 / 1.00 /
0.97 / 1.01; ragged 1.01 / 1.00 / 0.99 / 1.00; spike 0.96 / 0.95 / 0.95 / 1.10; offsets 0.99 / 1.02 / 0.65 / 1.05; the finite elements of the NaN
cases 1.00 / 1.12 / 0.95 / 1.07."""
import json
import os

import numpy as np
import pytest
import torch

import attn_stream_split_bwd_cases as cases
from attn_stream_bwd_ref import keep_mask, mha_train
from attn_stream_split_bwd_ref import mha3_train
from test_gpu_attn_stream_split import worst

pytestmark = pytest.mark.gpu
TENSORS = cases.TENSORS
REPORT = {}
X3 = "bf16x3"


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
        with open(os.path.join(d, "attn_stream_split_bwd.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def bits(t):
    return t.contiguous().view(torch.int32)


def run(c, dev, layout="three", seed=cases.SEED, precision=X3):
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
    kw = dict(scale=c["scale"], dropout_p=c["p"], seed=seed, site=cases.SITE, precision=precision)
    ctx, stats = kernels.attn_stream_train(q, k, v, sb, c["heads"], **kw)
    dq, dk, dv = kernels.attn_stream_backward(q, k, v, ctx, g, stats, sb, c["heads"], **kw)     # (R, 3 D) outputs
    return dict(ctx=ctx, dq=dq, dk=dk, dv=dv, stats=stats)


def check_family(name, fam, dev, layouts=("three",)):
    yard = cases.yardsticks(fam)
    ratio = dict.fromkeys(TENSORS, 0.0)
    for c in fam:
        s64 = cases.spec(c)[0]
        for lay in layouts:
            got = run(c, dev, lay)
            for t in TENSORS:
                ratio[t] = max(ratio[t], worst(got[t], s64[t], yard[t], (c["name"], lay, t)))
    REPORT[name] = dict(err_over_yardstick=ratio, yardstick=yard, cases=len(fam))
    print(f"attn_stream_split_bwd {name}: " + ", ".join(f"{t} {ratio[t]:.3f} yardsticks ({yard[t]:.3e})" for t in TENSORS) + f", {len(fam)} cases")
    return ratio


@pytest.mark.parametrize("T", (64, 200, 321))
def test_exact_small_integers(dev, T):
    """The lane maps of all seven products and the transposed operands on data that every plane and accumulator holds exactly.  Keys come
    in pairs (a, b = a with a balanced half of its +-1 entries flipped: a . b = 0); query i is 4 (a + b) of the pair sigma(i), so at scale 1
    its logits are 512 at a and b and at most about 300 elsewhere: alpha = 1/2 on the pair, every other weight underflows to 0, m = 512,
    l = 2.  V is integers in -3 .. 3 and dctx in -1 .. 1, so ctx, dA, delta are (half-)integers, dS = dctx . (v_a - v_b) / 4 at a (its
    negative at b) fits hi + lo, and dQ = dS (k_a - k_b), dK = sum dS q, dV = sum dctx / 2 are exact.  A fragment in another row order
    than the weights', or a plane read at another column, gives other numbers."""
    from summarizer_amd import kernels
    rng = np.random.default_rng(500 + T)
    D, heads, dh = 256, 2, 128
    npair = T // 2
    k = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(T, D))
    for h in range(heads):
        for t in range(npair):
            w = np.ones(dh, dtype=np.float32)
            w[rng.permutation(dh)[:dh // 2]] = -1.0
            k[2 * t + 1, h * dh:(h + 1) * dh] = k[2 * t, h * dh:(h + 1) * dh] * w
    sigma = rng.integers(0, npair, size=(T, heads))
    q = np.concatenate([4.0 * (k[2 * sigma[:, h], h * dh:(h + 1) * dh] + k[2 * sigma[:, h] + 1, h * dh:(h + 1) * dh]) for h in range(heads)], axis=1)
    v = rng.integers(-3, 4, size=(T, D)).astype(np.float32)
    g = rng.integers(-1, 2, size=(T, D)).astype(np.float32)
    want = {t: np.zeros((T, D)) for t in TENSORS}
    for h in range(heads):
        cols = slice(h * dh, (h + 1) * dh)
        s = q[:, cols].astype(np.float64) @ k[:, cols].T
        A = np.zeros((T, T))
        A[np.arange(T), 2 * sigma[:, h]] = 0.5
        A[np.arange(T), 2 * sigma[:, h] + 1] = 0.5
        assert (s[A > 0] == 512).all() and (s[A == 0] <= 512 - 110).all()          # exp(-110) is below the smallest float32
        ctx = A @ v[:, cols]
        dS = A * (g[:, cols].astype(np.float64) @ v[:, cols].T - (g[:, cols] * ctx).sum(axis=1)[:, None])
        want["ctx"][:, cols], want["dq"][:, cols], want["dk"][:, cols], want["dv"][:, cols] = ctx, dS @ k[:, cols], dS.T @ q[:, cols], A.T @ g[:, cols]
    assert np.abs(want["dq"]).max() > 4 and np.abs(want["dk"]).max() > 4
    c = dict(name=f"exact_T{T}", lens=[T], D=D, heads=heads, scale=1.0, q=q, k=k, v=v, dctx=g, p=0.0)
    for lay in ("three", "packed"):
        got = run(c, dev, lay)
        for t in TENSORS:
            assert np.array_equal(got[t].cpu().numpy().astype(np.float64), want[t]), (T, lay, t)
        st = got["stats"].cpu().numpy()
        assert (st[:, :, 0] == 512.0).all() and (st[:, :, 1] == 2.0).all(), (T, lay)


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


def test_p0_has_the_bits_of_the_scoring_call(dev):
    from summarizer_amd import kernels
    for c0 in (cases.fwd.case("fwd", (1, 64, 65, 200, 3, 129), 256, 2, 21), cases.fwd.case("fwd40", (129, 70), 80, 2, 22)):
        sb = kernels.SeqBatch.get(c0["lens"], dev)
        q, k, v = (torch.from_numpy(c0[n]).to(dev) for n in "qkv")
        plain, lse = kernels.attn_stream(q, k, v, sb, c0["heads"], want_lse=True, precision=X3)
        ctx, stats = kernels.attn_stream_train(q, k, v, sb, c0["heads"], dropout_p=0.0, seed=5, site=3, precision=X3)
        assert torch.equal(bits(ctx), bits(plain)), "p = 0 changed the bits of ctx"
        got = stats[:, :, 0].double() + torch.log(stats[:, :, 1].double())
        assert float((got - lse.double()).abs().max()) <= 1e-5 * float(lse.abs().max())


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_masks_bit_by_bit(dev, p):
    """T = 65 behind a first video of 3 rows, dh = 8, 9 heads (D = 72), Q = 0 so that alpha = 1 / T.
    A: K = 0, V = dctx = the 65 x 72 identity.  Head j // 8 sees key j alone in its column j % 8: ctx[i, j] != 0 <=> keep(i, j // 8, j), the
       forward's masks; and query i alone has a gradient in column i of head i // 8: dV[j, i] != 0 <=> keep(i, i // 8, j), the dK / dV
       pass's masks.  The kept entries are 1 / (T (1 - p)) to the 2^-16 of a weight split into two planes.
    B: K = the identity, V = dctx = ones.  dQ[i, j] = dS(i, head j // 8, key j) = (scale / T) (keep ? 8 / (1 - p) : 0 - delta_i) with delta_i
       strictly between: positive <=> keep(i, j // 8, j), the dQ pass's masks (rows of a head that kept or dropped every key apart)."""
    from summarizer_amd import kernels
    T, heads, lead = 65, 9, 3
    D = 8 * heads
    sb = kernels.SeqBatch.get([lead, T], dev)
    eye = np.zeros((lead + T, D), dtype=np.float32)
    eye[lead + np.arange(T), np.arange(T)] = 1.0
    eye_t = torch.from_numpy(eye).to(dev)
    z, ones = torch.zeros(lead + T, D, device=dev), torch.ones(lead + T, D, device=dev)
    kw = dict(dropout_p=p, seed=cases.SEED, site=cases.SITE, precision=X3)
    keep = np.stack([keep_mask(cases.SEED, cases.SITE, p, lead, T, heads, h) for h in range(heads)])          # (heads, query, key)
    assert 0.3 * p < 1.0 - keep.mean() < 2.0 * p
    want = 1.0 / T / (1.0 - float(np.float32(p)))
    # A
    ctx, stats = kernels.attn_stream_train(z, z, eye_t, sb, heads, **kw)
    _, _, dv = kernels.attn_stream_backward(z, z, eye_t, ctx, eye_t, stats, sb, heads, **kw)
    ctx, dv = ctx.cpu().numpy()[lead:], dv.cpu().numpy()[lead:]
    kf = np.stack([keep[j // 8][:, j] for j in range(T)], axis=1)                                            # [i, j] = keep(i, j // 8, j)
    assert np.array_equal(ctx[:, :T] != 0, kf), (p, "forward: kept entries differ from recipes.dropout_keep")
    assert np.abs(ctx[:, :T][kf] - want).max() <= 2.0 ** -16 * want and not ctx[:, T:].any()
    kb = np.stack([keep[i // 8][i, :] for i in range(T)], axis=1)                                            # [j, i] = keep(i, i // 8, j)
    assert np.array_equal(dv[:, :T] != 0, kb), (p, "dK / dV pass: kept entries differ from recipes.dropout_keep")
    assert np.abs(dv[:, :T][kb] - want).max() <= 2.0 ** -16 * want and not dv[:, T:].any()
    # B
    ctx, stats = kernels.attn_stream_train(z, eye_t, ones, sb, heads, **kw)
    dq, _, _ = kernels.attn_stream_backward(z, eye_t, ones, ctx, ones, stats, sb, heads, **kw)
    dq = dq.cpu().numpy()[lead:, :T]
    n_kept = np.stack([keep[j // 8].sum(axis=1) for j in range(T)], axis=1)                                  # [i, j]: keys head j // 8 kept for query i
    mixed = (n_kept > 0) & (n_kept < T)
    assert mixed.mean() > 0.9
    assert np.array_equal((dq > 0)[mixed], kf[mixed]) and (dq[mixed] != 0).all(), (p, "dQ pass: masks differ from recipes.dropout_keep")


def test_determinism_scratch_and_capture(dev):
    from summarizer_amd import kernels
    c = cases.with_grad(cases.fwd.case("det", (1, 64, 65, 200, 3, 129), 256, 2, 21), 0.1)
    a, b = run(c, dev), run(c, dev)
    for t in TENSORS + ("stats",):
        assert torch.equal(bits(a[t]), bits(b[t])), t
    other = run(c, dev, seed=cases.SEED + 1)
    assert not torch.equal(bits(other["dq"]), bits(a["dq"])), "another seed drew the same masks"
    sb = kernels.SeqBatch.get(c["lens"], dev)
    q, k, v, g = (torch.from_numpy(c[n]).to(dev) for n in ("q", "k", "v", "dctx"))
    kw = dict(dropout_p=0.1, seed=cases.SEED, site=cases.SITE, precision=X3)
    # the backward on a workspace and outputs pre-filled with 0xFF bytes
    nb = kernels.attn_stream_backward_workspace_bytes(256, 2, sb, precision=X3)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((sb.n_rows, 3 * 256), float("nan"), device=dev)
    got = kernels.attn_stream_backward(q, k, v, a["ctx"], g, a["stats"], sb, 2, out=out, ws=ws, **kw)
    for o, t in zip(got, ("dq", "dk", "dv")):
        assert torch.equal(bits(o), bits(a[t])), (t, "the result depends on what the workspace held")

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


def test_nan_rules(dev):
    """A NaN in one K row, one Q row, one V row, one dctx row: NaN positions as the float64 specification has them, the finite elements
    inside the gate (yardstick: the bf16x3 specification on the same inputs), nothing outside the video and nothing in the other head."""
    c = cases.with_grad(cases.fwd.case("nan", (70, 130, 40), 64, 2, 11), 0.1)
    base = run(c, dev)
    fam = []
    for which, row in (("k", 150), ("q", 100), ("v", 120), ("dctx", 199)):
        d = dict(c, name=f"nan3_{which}_{row}", **{which: c[which].copy()})
        d[which][row, 40] = np.nan                            # head 1
        fam.append(d)
    yard = cases.yardsticks(fam)
    ratio = dict.fromkeys(TENSORS, 0.0)
    for d in fam:
        s64, _, s3 = cases.spec(d)
        got = run(d, dev)
        for t in TENSORS:
            assert np.array_equal(np.isnan(s3[t]), np.isnan(s64[t])), (d["name"], t)
            ratio[t] = max(ratio[t], worst(got[t], s64[t], yard[t], (d["name"], t)))
            for lo, hi in ((0, 70), (200, 240)):              # the other videos: not a bit
                assert torch.equal(bits(got[t][lo:hi]), bits(base[t][lo:hi])), (d["name"], t)
            assert not bool(torch.isnan(got[t][:, :32]).any()), (d["name"], t, "NaN crossed into head 0")
    REPORT["nan"] = dict(err_over_yardstick=ratio, yardstick=yard, cases=len(fam))
    print("attn_stream_split_bwd nan: " + ", ".join(f"{t} {ratio[t]:.3f} yardsticks ({yard[t]:.3e})" for t in TENSORS))


def test_offsets_past_2_31_bytes(dev):
    """704 videos of 256 frames at D = 1024 in the (R, 3 D) layout: both buffers are 2.2e9 bytes and each of the backward's seven plane
    blocks 7.4e8, so the last videos lie past 2^31 bytes in the operands, the outputs and the workspace.  The last three are compared."""
    from summarizer_amd import kernels
    n_vid, T, D, heads = 704, 256, 1024, 8
    rows = n_vid * T
    assert rows * 3 * D * 4 > 2 ** 31
    sb = kernels.SeqBatch.get([T] * n_vid, dev)
    nb = kernels.attn_stream_backward_workspace_bytes(D, heads, sb, precision=X3)
    assert nb > 2 * 2 ** 31 and kernels.attn_stream_workspace_bytes(D, heads, sb, precision=X3) > 2 ** 31
    gen = torch.Generator(device=dev).manual_seed(5)
    buf = torch.randn(rows, 3 * D, device=dev, generator=gen)
    g = torch.randn(rows, D, device=dev, generator=gen)
    out = torch.empty(rows, 3 * D, device=dev)
    kw = dict(dropout_p=0.1, seed=cases.SEED, site=cases.SITE, precision=X3)
    q, k, v = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:]
    ctx, stats = kernels.attn_stream_train(q, k, v, sb, heads, **kw)
    dq, dk, dv = kernels.attn_stream_backward(q, k, v, ctx, g, stats, sb, heads, out=out, **kw)
    n = 3 * T
    tail, gt = buf[-n:].cpu().numpy(), g[-n:].cpu().numpy()
    # the specifications on the last three videos alone; their masks are indexed by the packed row
    a = (tail[:, :D], tail[:, D:2 * D], tail[:, 2 * D:], gt, [T] * 3, heads, 1.0 / np.sqrt(D // heads), 0.1, cases.SEED, cases.SITE)
    s64, s3 = mha_train(*a, row0=rows - n), mha3_train(*a, row0=rows - n)
    ratio = {}
    for t, got in (("ctx", ctx), ("dq", dq), ("dk", dk), ("dv", dv)):
        ratio[t] = worst(got[-n:], s64[t], float(np.abs(s3[t] - s64[t]).max()), ("offsets", t))
    REPORT["offsets"] = dict(err_over_yardstick=ratio)
    print("attn_stream_split_bwd offsets: " + ", ".join(f"{t} {ratio[t]:.3f} yardsticks" for t in TENSORS))
    del buf, g, out, ctx, stats, dq, dk, dv
    torch.cuda.empty_cache()


def test_fp32_calls_unchanged(dev):
    """precision="fp32" is the call without the argument, bit for bit, and differs from the bf16x3 call."""
    c = cases.with_grad(cases.fwd.case("same", (70, 130, 257), 256, 2, 31), 0.1)
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(c["lens"], dev)
    q, k, v, g = (torch.from_numpy(c[n]).to(dev) for n in ("q", "k", "v", "dctx"))
    kw = dict(dropout_p=0.1, seed=cases.SEED, site=cases.SITE)
    ctx, stats = kernels.attn_stream_train(q, k, v, sb, 2, **kw)
    grads = kernels.attn_stream_backward(q, k, v, ctx, g, stats, sb, 2, **kw)
    old = dict(zip(TENSORS + ("stats",), (ctx,) + tuple(grads) + (stats,)))
    same, x3 = run(c, dev, precision="fp32"), run(c, dev)
    for t in TENSORS + ("stats",):
        assert torch.equal(bits(old[t]), bits(same[t])), t
        assert not torch.equal(bits(old[t]), bits(x3[t])), t
    assert kernels.attn_stream_backward_workspace_bytes(256, 2, sb) == kernels.attn_stream_backward_workspace_bytes(256, 2, sb, precision="fp32")


def test_refusals(dev):
    from summarizer_amd import kernels
    from summarizer_amd._lib import SumkError
    sb = kernels.SeqBatch.get([10], dev)
    for D in (8, 72, 512):
        x = torch.zeros(10, D, device=dev)
        st = torch.zeros(10, 2, 2, device=dev)
        with pytest.raises(SumkError, match=f"head width {D // 2}"):
            kernels.attn_stream_train(x, x, x, sb, 2, precision=X3)
        with pytest.raises(SumkError, match=f"head width {D // 2}"):
            kernels.attn_stream_backward(x, x, x, x, x, st, sb, 2, precision=X3)
    x = torch.zeros(10, 64, device=dev)
    for bad in ("bf16x6", "bf16", "fp16"):
        with pytest.raises(SumkError):
            kernels.attn_stream_train(x, x, x, sb, 2, precision=bad)
        with pytest.raises(SumkError):
            kernels.attn_stream_backward(x, x, x, x, x, torch.zeros(10, 2, 2, device=dev), sb, 2, precision=bad)
