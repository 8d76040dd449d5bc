"""GPU: the streaming attention in bf16x3 (csrc/attn_stream_split.hip through kernels.attn_stream(..., precision="bf16x3")) against the
float64 specification tests/attn_stream_ref.py on the unsplit inputs, element by element of ctx and of lse.

The gate: a family's yardstick is the largest |bf16x3 specification - float64 specification| over its cases (tests/attn_stream_split_ref.py:
what the arithmetic costs, ctx and lse apart), and every element must lie within 4 yardsticks (at least 2 fp32 ulps of the value) of the
float64 reference.  Nothing is left out of a comparison; NaN positions must agree exactly.  tests/test_attn_stream_split_host.py shows
that the yardsticks are not blown up (at most 4 x 2^8 fp32 yardsticks) and that the gate catches a dropped plane product, a one-plane P,
a natural-order V fragment and a lost key.

Families (tests/attn_stream_split_cases.py): strips at head widths 8, 40, 104, 128 in both operand layouts, ragged batches, spikes; NaN
rules, determinism / poisoned workspace / graph capture, a buffer and planes past 2^31 bytes, the refusals, and the untouched fp32 call.
Every family prints its worst error / yardstick and keeps it in REPORT ($SUMK_REPORT_DIR/attn_stream_split.json when set).
Measured on MI355X (2026-10-21), worst error / yardstick, ctx / lse (4 is the limit): strips D32 h4 0.97 / 0.99, D80 h2 1.00 / 1.00, D208 h2
0.93 / 0.93, D128 h1 1.16 / 0.94, D256 h2 1.05 / 0.96; ragged 1.00 / 0.95; spike 0.96 / 1.00; offsets 1.07 / 1.00; the finite elements of
the NaN cases 1.08 / 0.97."""
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_stream_cases as base
import attn_stream_split_cases as cases

pytestmark = pytest.mark.gpu
MULT = 4.0
REPORT = {}
spec = cases.spec


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
        with open(os.path.join(d, "attn_stream_split.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def run(c, dev, layout="three", want_lse=True, precision="bf16x3"):
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(c["lens"], dev)
    D = c["D"]
    if layout == "three":
        q, k, v = (torch.from_numpy(c[n]).to(dev) for n in "qkv")
    else:
        buf = torch.from_numpy(np.concatenate([c["q"], c["k"], c["v"]], axis=1)).to(dev)
        q, k, v = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:]
    return kernels.attn_stream(q, k, v, sb, c["heads"], scale=c["scale"], want_lse=want_lse, precision=precision)


def worst(got, ref64, yard, what):
    """max over elements of |got - ref| / yardstick after asserting every element inside max(4 yardsticks, 2 ulps).  got: a tensor or an array."""
    got = got.double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), (what, "NaN positions differ")
    ok = ~np.isnan(ref64)
    err = np.abs(got[ok] - ref64[ok])
    gate = np.maximum(MULT * yard, 2.0 * np.spacing(np.abs(ref64[ok]).astype(np.float32)).astype(np.float64))
    bad = err > gate
    assert not bad.any(), (what, float(err.max()), yard, int(bad.sum()))
    return float(err.max() / yard) if yard > 0 else 0.0


def check_family(name, fam, dev, layouts=("three",)):
    yc, yl = cases.yardsticks(fam)[:2]
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
    print(f"attn_stream_split {name}: ctx {rc:.3f} yardsticks ({yc:.3e}), lse {rl:.3f} yardsticks ({yl:.3e}), {len(fam)} cases")


@pytest.mark.parametrize("T", (64, 200, 321))
def test_exact_small_integers(dev, T):
    """The lane maps of both products on data that every plane and accumulator holds exactly: keys are +-1 sign patterns, query i is twice
    the key sigma(i) (logit 256 there, at most about 100 elsewhere: every other weight underflows to 0 at scale 1), V small integers.  Then
    ctx[i] = V[sigma(i)] and lse = 256 to the bit; a V fragment in another key order than the weights' gives other rows."""
    rng = np.random.default_rng(400 + T)
    D, heads = 256, 2
    k = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(T, D))
    sigma = np.stack([rng.permutation(T) for _ in range(heads)], axis=1)            # (T, heads)
    q = np.concatenate([2.0 * k[sigma[:, h], h * 128:(h + 1) * 128] for h in range(heads)], axis=1)
    v = rng.integers(-200, 201, size=(T, D)).astype(np.float32)
    c = dict(name=f"exact_T{T}", lens=[T], D=D, heads=heads, scale=1.0, q=q, k=k, v=v)
    s = np.stack([q[:, h * 128:(h + 1) * 128] @ k[:, h * 128:(h + 1) * 128].T for h in range(heads)])
    assert (np.sort(s, axis=2)[:, :, -2] <= 256 - 110).all()                        # exp(-110) / 1 is below half an ulp of 1; times 200 T too
    want = np.concatenate([v[sigma[:, h], h * 128:(h + 1) * 128] for h in range(heads)], axis=1)
    for lay in ("three", "packed"):
        ctx, lse = run(c, dev, lay)
        assert np.array_equal(ctx.cpu().numpy(), want), (T, lay)
        assert bool((lse == 256.0).all()), (T, lay)


@pytest.mark.parametrize("D,heads", cases.STRIP_SHAPES)
def test_strips(dev, D, heads):
    check_family(f"strips_D{D}_h{heads}", cases.strips(D, heads), dev, layouts=("three", "packed"))


def test_ragged(dev):
    check_family("ragged", base.ragged(), dev, layouts=("three", "packed"))


def test_spike(dev):
    check_family("spike", base.spikes(), dev)


def test_nan_rules(dev):
    """NaN positions as the float64 specification has them, the other videos bit-equal to the run without NaN, and every finite element
    -- those of the poisoned video included -- inside the family's gate."""
    c = base.case("nan", (70, 130, 40), 64, 2, 11)
    bits = lambda t: t.view(torch.int32)
    b_ctx, b_lse = run(c, dev)
    fam = []
    for which, row, col in (("q", 100, None), ("k", 150, 40), ("v", 199, None), ("v", 71, 5)):
        d = dict(c, name=f"nan_{which}_{row}_{col}", **{which: c[which].copy()})
        if col is None:
            d[which][row] = np.nan
        else:
            d[which][row, col] = np.nan
        fam.append(d)
    yc, yl = cases.yardsticks(fam)[:2]
    rc = rl = 0.0
    out = {}
    for d in fam:
        got, lse = run(d, dev)
        assert np.array_equal(np.isnan(spec(d)[4]), np.isnan(spec(d)[0])) and np.array_equal(np.isnan(spec(d)[5]), np.isnan(spec(d)[1])), d["name"]
        rc = max(rc, worst(got, spec(d)[0], yc, (d["name"], "ctx")))
        rl = max(rl, worst(lse, spec(d)[1], yl, (d["name"], "lse")))
        for lo, hi in ((0, 70), (200, 240)):              # the other videos: not a bit
            assert torch.equal(bits(got[lo:hi]), bits(b_ctx[lo:hi])) and torch.equal(bits(lse[lo:hi]), bits(b_lse[lo:hi])), d["name"]
        out[d["name"]] = (got.cpu().numpy(), lse.cpu().numpy())
    REPORT["nan"] = dict(ctx_err_over_yardstick=rc, lse_err_over_yardstick=rl, ctx_yardstick=yc, lse_yardstick=yl, cases=len(fam))
    print(f"attn_stream_split nan: ctx {rc:.3f} yardsticks ({yc:.3e}), lse {rl:.3f} yardsticks ({yl:.3e}), {len(fam)} cases")
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
    c = base.case("det", (1, 64, 65, 200, 3, 129), 256, 2, 21)
    sb = kernels.SeqBatch.get(c["lens"], dev)
    q, k, v = (torch.from_numpy(c[n]).to(dev) for n in "qkv")
    bits = lambda t: t.view(torch.int32)
    call = lambda q, k, v: kernels.attn_stream(q, k, v, sb, 2, want_lse=True, precision="bf16x3")
    a, la = call(q, k, v)
    b, lb = call(q, k, v)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(la), bits(lb))
    # workspace and outputs pre-filled with 0xFF bytes, through the raw entry
    lib = __import__("summarizer_amd._lib", fromlist=["load"]).load()
    nb = kernels.attn_stream_workspace_bytes(256, 2, sb, precision="bf16x3")
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    ctx = torch.empty(sb.n_rows, 256, device=dev); ctx.view(torch.int32).fill_(-1)
    lse = torch.empty(sb.n_rows, 2, device=dev); lse.view(torch.int32).fill_(-1)
    rc = lib.sumk_attn_stream_split(q.data_ptr(), 256, k.data_ptr(), 256, v.data_ptr(), 256, 256, 2, sb.n_seq, sb.off_host_p, sb.off_dev_p,
                                    1.0 / math.sqrt(128), kernels.PRECISIONS["bf16x3"], ctx.data_ptr(), 256, lse.data_ptr(), ws.data_ptr(),
                                    nb, kernels._stream())
    assert rc == 0, lib.sumk_last_error()
    assert torch.equal(bits(ctx), bits(a)) and torch.equal(bits(lse), bits(la))
    # one call captured into a graph, replayed twice on changed inputs
    qs, ks, vs = q.clone(), k.clone(), v.clone()
    call(qs, ks, vs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gc, gl = call(qs, ks, vs)
    for seed in (22, 23):
        c2 = base.case("det2", c["lens"], 256, 2, seed)
        for dst, n in ((qs, "q"), (ks, "k"), (vs, "v")):
            dst.copy_(torch.from_numpy(c2[n]))
        graph.replay()
        torch.cuda.synchronize()
        e, le = call(qs, ks, vs)
        assert torch.equal(bits(gc), bits(e)) and torch.equal(bits(gl), bits(le)), seed
        assert not torch.equal(bits(e), bits(a))


def test_offsets_past_2_31_bytes(dev):
    """2800 videos of 64 frames at D = 1024: the (rows, 3 D) buffer and the planes in the workspace are 2.2e9 bytes each, so the last
    videos' offsets into either do not fit 31 bits.  The last three videos are compared."""
    from summarizer_amd import kernels
    n_vid, T, D, heads = 2800, 64, 1024, 8
    rows = n_vid * T
    assert rows * 3 * D * 4 > 2 ** 31
    sb = kernels.SeqBatch.get([T] * n_vid, dev)
    assert kernels.attn_stream_workspace_bytes(D, heads, sb, precision="bf16x3") > 2 ** 31
    g = torch.Generator(device=dev).manual_seed(5)
    buf = torch.randn(rows, 3 * D, device=dev, generator=g)
    ctx, lse = kernels.attn_stream(buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:], sb, heads, want_lse=True, precision="bf16x3")
    tail = buf[-3 * T:].cpu().numpy()
    c = dict(name="offsets_tail", lens=[T] * 3, D=D, heads=heads, scale=None, q=tail[:, :D], k=tail[:, D:2 * D], v=tail[:, 2 * D:])
    yc, yl = cases.yardsticks([c])[:2]
    rc = worst(ctx[-3 * T:], spec(c)[0], yc, "offsets ctx")
    rl = worst(lse[-3 * T:], spec(c)[1], yl, "offsets lse")
    REPORT["offsets"] = dict(ctx_err_over_yardstick=rc, lse_err_over_yardstick=rl)
    print(f"attn_stream_split offsets: ctx {rc:.3f} yardsticks, lse {rl:.3f} yardsticks")
    del buf, ctx, lse
    torch.cuda.empty_cache()


def test_refusals(dev):
    from summarizer_amd import _lib, kernels
    from summarizer_amd._lib import SumkError
    lib = _lib.load()
    PAT = 0x5A5A5A5A
    X3 = kernels.PRECISIONS["bf16x3"]

    def call(D, heads, lens, precision=X3, short=0, want=-1, msg=b""):
        rows = sum(lens)
        off_host = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        off_dev = torch.from_numpy(off_host).to(dev)
        q = torch.zeros(rows, D, device=dev)
        ctx = torch.empty(rows, D, device=dev); ctx.view(torch.int32).fill_(PAT)
        lse = torch.empty(rows, heads, device=dev); lse.view(torch.int32).fill_(PAT)
        need = int(lib.sumk_attn_stream_split_workspace_bytes(D, heads, len(lens), _lib.host_i32(off_host), precision))
        assert (need > 0) == (want != -1), (need, want)
        nb = max(need, 256)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev); ws.fill_(0x5A)
        rc = lib.sumk_attn_stream_split(q.data_ptr(), D, q.data_ptr(), D, q.data_ptr(), D, D, heads, len(lens), _lib.host_i32(off_host),
                                        off_dev.data_ptr(), 0.25, precision, ctx.data_ptr(), D, lse.data_ptr(), ws.data_ptr(), nb - short,
                                        kernels._stream())
        torch.cuda.synchronize()
        assert rc == want, (rc, want, lib.sumk_last_error())
        if want != 0:
            assert msg in lib.sumk_last_error(), (msg, lib.sumk_last_error())
            assert bool((ctx.view(torch.int32) == PAT).all()) and bool((lse.view(torch.int32) == PAT).all()), msg
            assert bool((ws == 0x5A).all()), msg
        return need
    need = call(64, 2, [10], want=0)
    call(8, 2, [10], msg=b"head width 4")
    call(72, 2, [10], msg=b"head width 36")
    call(512, 2, [10], msg=b"head width 256")
    call(64, 2, [10], precision=kernels.PRECISIONS["bf16x6"], msg=b"precision=2")
    call(64, 2, [10], precision=kernels.PRECISIONS["fp32"], msg=b"precision=0")
    call(64, 2, [10], short=1, want=-2, msg=b"workspace %d < required %d" % (need - 1, need))
    # the Python wrapper: bf16x6 and unknown names raise
    sb = kernels.SeqBatch.get([10], dev)
    q = torch.zeros(10, 64, device=dev)
    for bad in ("bf16x6", "bf16", "fp16"):
        with pytest.raises(SumkError):
            kernels.attn_stream(q, q, q, sb, 2, precision=bad)
        with pytest.raises(SumkError):
            kernels.attn_stream_workspace_bytes(64, 2, sb, precision=bad)
    for D in (8, 72, 512):
        with pytest.raises(SumkError, match="head width"):
            kernels.attn_stream(torch.zeros(10, D, device=dev), torch.zeros(10, D, device=dev), torch.zeros(10, D, device=dev), sb, 2,
                                precision="bf16x3")


def test_fp32_call_unchanged(dev):
    """precision="fp32" is the call without the argument, bit for bit (ctx and lse), and differs from the bf16x3 call."""
    from summarizer_amd import kernels
    c = base.case("same", (70, 130, 257), 256, 2, 31)
    sb = kernels.SeqBatch.get(c["lens"], dev)
    q, k, v = (torch.from_numpy(c[n]).to(dev) for n in "qkv")
    bits = lambda t: t.view(torch.int32)
    a, la = kernels.attn_stream(q, k, v, sb, 2, want_lse=True)
    b, lb = kernels.attn_stream(q, k, v, sb, 2, want_lse=True, precision="fp32")
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(la), bits(lb))
    assert kernels.attn_stream_workspace_bytes(256, 2, sb) == kernels.attn_stream_workspace_bytes(256, 2, sb, precision="fp32")
    x, lx = kernels.attn_stream(q, k, v, sb, 2, want_lse=True, precision="bf16x3")
    assert not torch.equal(bits(a), bits(x))
