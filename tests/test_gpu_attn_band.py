"""GPU: local attention on the band (csrc/attn_band.hip: sumk_attn_band, sumk_vasnet_forward_band), kernels.attn_band,
VASNet(local_attention="band") and a Summarizer in front of the long-video tail.

Gates
  * sumk_attn_band against the float64 band-only specification tests/attn_band_ref.py (pinned to the dense oracle in
    tests/test_attn_band_host.py): NaN positions EQUAL, elsewhere max |hip - f64| <= max(4 x max |spec_f32 - f64|, 2 x 2^-23 x max |f64|)
    per case and quantity -- the project's standing gate (4 x the yardstick of the same specification run in float32, floor 2 fp32 ulps).
    The float32 run sums both products as one accumulator chain per element, the rule of oracle/torch_port.mm_chain for the library's
    exact-fp32 MFMA GEMMs (tests/attn_band_ref.py says why).  With numpy's blocked float32 products as the yardstick instead -- the first
    form of this file -- the D = 64 cases passed and every D = 256 case with w >= 31 missed: ctx 1.41e-6 .. 1.88e-6 against gates of
    1.14e-6 .. 1.68e-6, alpha 4.0e-7 .. 4.9e-7 against 3.0e-7 .. 5.2e-7 (1.1 .. 1.35 x the gate); a chain over K = 256 terms rounds
    about 4 x what a blocked sum does, and the kernel is such a chain (the dense path's, bit for bit).
  * model level: scores within 1e-4 of oracle.vasnet_np.vasnet_forward(..., aperture=w, dtype=float64), the project's parity gate for scores.
Every test prints its worst figure and keeps it in REPORT (written to $SUMK_REPORT_DIR/attn_band.json when set).

Measured on MI355X (worst over the 36 cases of test 1): ctx error / yardstick 1.42, alpha 1.59 (limit 4); row sums of alpha within 1.5e-7
of 1; offsets past 2^31 bytes (T = 262 144): error 2.3e-7, yardstick 2.6e-7; model scores at most 1.8e-6 from float64 (gate 1e-4) and at
most 1.5e-6 from the dense path.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import attn_band_ref
import kts_ref
from oracle import vasnet_np

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
REPORT = []
LENS = [1, 65, 200, 64, 333, 2]
ZERO_ROW = 1 + 65 + 200 + 64 + 100                       # the planted all-zero query row: row 100 of the 333-step video
WINDOWS = [0, 1, 31, 32, 63, 64, 100, 332, 5000]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for r in REPORT:
        print("ATTN-BAND-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "attn_band.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


# ------------------------------------------------------------------------------------------------ inputs, references and calls
@functools.lru_cache(maxsize=None)
def _qkv(D):
    """(rows, 3 D) float32 [Q | K | V] ~ N(0, 1) for LENS with the planted zero query row; read-only."""
    x = np.random.default_rng(4100 + D).standard_normal((sum(LENS), 3 * D)).astype(np.float32)
    x[ZERO_ROW, :D] = 0.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _spec(D, w, ignore_self):
    """(ctx64, alpha64, ctx32, alpha32) of the specification -- computed once per case, shared by the tests, never modified."""
    x = _qkv(D)
    out = attn_band_ref.band_attention(x[:, :D], x[:, D:2 * D], x[:, 2 * D:], LENS, w, 1.0 / np.sqrt(D), ignore_self)
    out += attn_band_ref.band_attention(x[:, :D], x[:, D:2 * D], x[:, 2 * D:], LENS, w, 1.0 / np.sqrt(D), ignore_self, dtype=np.float32)
    for a in out:
        a.setflags(write=False)
    return out


def _gate(s64, s32):
    fin = ~np.isnan(s64)
    assert np.array_equal(fin, ~np.isnan(s32))
    if not fin.any():
        return 0.0, 0.0
    yard = float(np.abs(s32[fin].astype(np.float64) - s64[fin]).max())
    return yard, max(4 * yard, 2 * EPS * float(np.abs(s64[fin]).max()))


def _raw(dev, q, k, v, lens, w, scale, ignore_self, want_alpha=False, fill=255, ws_bytes=None, D=None, bufs=None):
    """sumk_attn_band on buffers of this test: workspace, ctx and alpha handed over filled with the byte `fill` (0xFF: NaN).
    Returns (rc, ctx, alpha or None, bytes needed).  bufs: (ws, ctx, alpha, device offsets) to reuse -- a call inside a graph capture
    allocates and copies nothing."""
    from summarizer_amd import _lib
    lib = _lib.load()
    D = q.shape[1] if D is None else D
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    off_dev = torch.from_numpy(off).to(dev) if bufs is None else bufs[3]
    need = lib.sumk_attn_band_workspace_bytes(D, len(lens), _lib.host_i32(off), w)
    nb = need if ws_bytes is None else ws_bytes
    if bufs is None:
        ws = torch.full((max(nb, 256),), fill, dtype=torch.uint8, device=dev)
        ctx = torch.full((q.shape[0], q.shape[1]), float("nan"), dtype=torch.float32, device=dev)
        alpha = torch.full((q.shape[0], 2 * w + 1), float("nan"), dtype=torch.float32, device=dev) if want_alpha else None
        for t in (ctx, alpha):
            if t is not None:
                t.view(torch.uint8).fill_(fill)
    else:
        ws, ctx, alpha = bufs[:3]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.sumk_attn_band(p(q), q.stride(0), p(k), k.stride(0), p(v), v.stride(0), D, len(lens), _lib.host_i32(off), p(off_dev), float(scale),
                            int(ignore_self), w, p(ctx), ctx.stride(0), p(alpha), p(ws), nb, st)
    if bufs is None:
        torch.cuda.synchronize()
    ctx._keep = (off_dev, ws)
    return rc, ctx, alpha, need


def _split(dev, D, x=None):
    """Q, K, V on the device: D = 64 as column blocks of ONE (rows, 3 D) tensor (leading dimension 3 D), otherwise three dense tensors."""
    t = torch.from_numpy(np.array(_qkv(D) if x is None else x)).to(dev)
    if D == 64:
        return t[:, :D], t[:, D:2 * D], t[:, 2 * D:]
    return t[:, :D].contiguous(), t[:, D:2 * D].contiguous(), t[:, 2 * D:].contiguous()


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("w", WINDOWS)
def test_attn_band_against_float64(dev, D, w):
    q, k, v = _split(dev, D)
    for ignore_self in (False, True):
        c64, a64, c32, a32 = _spec(D, w, ignore_self)
        rc, ctx, alpha, _ = _raw(dev, q, k, v, LENS, w, 1.0 / np.sqrt(D), ignore_self, want_alpha=True)
        assert rc == 0
        ctx, alpha = ctx.cpu().numpy(), alpha.cpu().numpy()
        yc, gc = _gate(c64, c32)
        ya, ga = _gate(a64, a32)
        fc, fa = ~np.isnan(c64), ~np.isnan(a64)
        ec = float(np.abs(ctx[fc] - c64[fc]).max()) if fc.any() else 0.0
        ea = float(np.abs(alpha[fa] - a64[fa]).max()) if fa.any() else 0.0
        rows_ok = ~np.isnan(a64).any(axis=1)
        es = float(np.abs(alpha[rows_ok].astype(np.float64).sum(axis=1) - 1.0).max()) if rows_ok.any() else 0.0
        REPORT.append({"case": f"f64_D{D}_w{w}_self{int(ignore_self)}", "ctx_error": ec, "ctx_yardstick": yc, "ctx_gate": gc, "alpha_error": ea,
                       "alpha_yardstick": ya, "alpha_gate": ga, "row_sum_error": es, "nan_rows": int((~rows_ok).sum())})
        print("attn_band D", D, "w", w, "ignore_self", ignore_self, "ctx err / yardstick / gate", ec, yc, gc, "alpha", ea, ya, ga, "row sums", es,
              "NaN rows", int((~rows_ok).sum()))
        assert np.array_equal(np.isnan(ctx), ~fc) and np.array_equal(np.isnan(alpha), ~fa)
        assert not rows_ok[ZERO_ROW]                                           # the planted row is all-masked
        assert ec <= gc and ea <= ga and es <= ga, (ec, gc, ea, ga, es)
        if w == 0 and not ignore_self:                                         # one key, weight 1: the context IS the value row
            vv = v.cpu().numpy()
            assert np.array_equal(ctx[rows_ok].view(np.int32), vv[rows_ok].view(np.int32))


# ------------------------------------------------------------------------------------------------ 2. isolation
@pytest.mark.parametrize("w", [31, 100])
def test_a_nan_video_stays_in_its_rows(dev, w):
    D, bad = 64, 3
    r0, r1 = sum(LENS[:bad]), sum(LENS[:bad + 1])
    q, k, v = _split(dev, D)
    rc, want, _, _ = _raw(dev, q, k, v, LENS, w, 0.125, False)
    x = np.array(_qkv(D))
    x[r0:r1] = np.nan
    qn, kn, vn = _split(dev, D, x)
    rc2, got, _, _ = _raw(dev, qn, kn, vn, LENS, w, 0.125, False)                # workspace and outputs pre-filled with 0xFF here, whatever the suite's mode
    assert rc == 0 and rc2 == 0
    want, got = want.cpu().numpy(), got.cpu().numpy()
    keep = np.ones(sum(LENS), dtype=bool); keep[r0:r1] = False
    assert np.isnan(got[r0:r1]).all()
    assert np.array_equal(got[keep].view(np.int32), want[keep].view(np.int32))
    assert int(np.isnan(want[keep]).any(axis=1).sum()) == 1                     # (only the planted row)
    REPORT.append({"case": f"isolation_w{w}", "rows_compared": int(keep.sum()), "mismatches": 0})


# ------------------------------------------------------------------------------------------------ 3. determinism and capture
def test_deterministic_and_captures(dev):
    D, w = 64, 40
    q, k, v = _split(dev, D)
    rc, a, aa, need = _raw(dev, q, k, v, LENS, w, 0.125, True, want_alpha=True)
    rc2, b, ab, _ = _raw(dev, q, k, v, LENS, w, 0.125, True, want_alpha=True, fill=0x5A)
    assert rc == 0 and rc2 == 0
    same = lambda s, t: torch.equal(s.view(torch.int32), t.view(torch.int32))
    assert same(a, b) and same(aa, ab)
    ws = torch.full((need,), 255, dtype=torch.uint8, device=dev)
    ctx, alpha = torch.zeros_like(a), torch.zeros_like(aa)
    off_dev = torch.from_numpy(np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rcg, _, _, _ = _raw(dev, q, k, v, LENS, w, 0.125, True, want_alpha=True, bufs=(ws, ctx, alpha, off_dev))
    assert rcg == 0
    for _ in range(2):
        ctx.fill_(7.0); alpha.fill_(7.0); ws.fill_(255)
        g.replay()
        torch.cuda.synchronize()
        assert same(ctx, a) and same(alpha, aa)
    REPORT.append({"case": "determinism_capture", "replays": 2, "mismatches": 0})


# ------------------------------------------------------------------------------------------------ 4. model level
MODEL_LENS = [1, 65, 300, 129]


def _models(dev, D, w, **kw):
    from summarizer_amd.models.vasnet import VASNet
    torch.manual_seed(100 + D + w)
    band = VASNet(input_size=D, attention_aperture=w, local_attention="band", **kw).eval()
    dense = VASNet(input_size=D, attention_aperture=w, **kw).eval()
    dense.load_state_dict(band.state_dict())
    return band.to(dev), dense.to(dev)


def _model_case(dev, D, w, tag, **kw):
    import recipes as R
    band, dense = _models(dev, D, w, **kw)
    params = {k: t.detach().cpu().numpy() for k, t in band.state_dict().items()}
    table = params.pop("pos_embed.weight", None)
    xs = [R.features(T, 1, D, 50 + T) for T in MODEL_LENS]
    x = torch.from_numpy(np.concatenate([a[:, 0] for a in xs])).to(dev)
    before = x.clone()
    with torch.no_grad():
        got = band.score_packed(x, MODEL_LENS).cpu().numpy()
        far = dense.score_packed(x, MODEL_LENS).cpu().numpy()
    assert torch.equal(x, before)                                               # score_packed never mutates its input
    want = np.concatenate([vasnet_np.vasnet_forward(a, params, aperture=w, pos_table=table, dtype=np.float64).reshape(-1) for a in xs])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    err = float(np.abs(got[fin] - want[fin]).max())
    dist = float(np.abs(got[fin] - far[fin]).max()) if np.array_equal(np.isnan(far), np.isnan(got)) else float("nan")
    REPORT.append({"case": f"model_{tag}_D{D}_w{w}", "error_vs_f64": err, "gate": 1e-4, "distance_to_dense_path": dist, "nan_rows": int((~fin).sum())})
    print("band model", tag, "D", D, "w", w, "max |score - f64|", err, "max |band - dense|", dist, "NaN rows", int((~fin).sum()))
    assert err <= 1e-4, err


@pytest.mark.parametrize("D", [64, 1024])
@pytest.mark.parametrize("w", [0, 16, 64])
def test_band_model_against_float64(dev, D, w):
    _model_case(dev, D, w, "plain")


def test_band_model_with_positions(dev):
    _model_case(dev, 64, 16, "positions", max_length=512)


def test_band_model_under_autograd_stays_dense(dev):
    """Training on the band is out of scope: a call that records a graph runs the dense masked path and still has gradients."""
    band, dense = _models(dev, 64, 16)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((130, 64)).astype(np.float32)).to(dev)
    band.train(); dense.train()
    torch.manual_seed(9); a = band.score_packed(x, [65, 65])
    assert a.requires_grad
    a.sum().backward()
    assert band.K.weight.grad is not None and torch.isfinite(band.K.weight.grad).all()


def test_summarizer_long_tail_with_a_band_model(dev):
    import summarizer_amd
    n, D, w = 5000, 64, 64
    band, dense = _models(dev, D, w)
    X = kts_ref.planted_features(n, D, 50, 0.05, 5000)[0]
    feats = [torch.from_numpy(X).to(dev)]
    kw = dict(kts="banded", device=True, tail="long", lmax=300, max_ncp=80)
    got = summarizer_amd.Summarizer(band, **kw).summarize_batch(feats)[0]
    want = summarizer_amd.Summarizer(dense, **kw).summarize_batch(feats)[0]
    torch.cuda.synchronize()
    assert int(got["status"]) == 0 and int(want["status"]) == 0
    assert int(got["n_segs"]) == int(want["n_segs"]) > 10
    assert torch.equal(got["change_points"], want["change_points"])
    assert torch.equal(got["machine_summary"], want["machine_summary"]) and 0 < float(got["machine_summary"].sum()) <= 0.15 * n + 1
    dist = float((got["scores"] - want["scores"]).abs().max())
    REPORT.append({"case": "summarizer_long_n5000", "n_segs": int(got["n_segs"]), "summary_frames": int(got["machine_summary"].sum()),
                   "distance_to_dense_path": dist})
    print("Summarizer long tail, band model: segments", int(got["n_segs"]), "summary frames", int(got["machine_summary"].sum()), "max |band - dense| scores", dist)


def test_trainer_test_with_a_band_model(dev, monkeypatch):
    """`Trainer.test` with hps.eval_tail = "long" on a fold with a 5000-step video: the band model scores through kernels.vasnet_forward_band
    and the fold stays on the device; correlation and F-scores agree with the same weights on the dense path (scores differ by ~1e-6, so
    the rank correlation moves in its last digits only; a key shot could flip on a tie: F-scores are held to 1e-3, not to equality)."""
    from summarizer_amd import kernels
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.hps import make_hps
    from test_gpu_corr_long import _fold_dataset
    ds, keys = _fold_dataset(), ["video_1", "video_2"]
    calls = []
    real = kernels.vasnet_forward_band
    monkeypatch.setattr(kernels, "vasnet_forward_band", lambda *a, **k: calls.append(a[1].n_rows) or real(*a, **k))
    res = {}
    for mode in ("band", "dense"):
        hps = make_hps(ds, [{"train_keys": [], "test_keys": keys}], epochs=1, eval_tail="long",
                       extra_params={"input_size": "64", "local": "16", "local_attention": mode})
        torch.manual_seed(78)
        t = VASNetTrainer(hps, hps.splits_files[0]).reset()
        assert t.model.local_attention == mode
        n = len(calls)
        res[mode] = t.test(0)
        assert (len(calls) > n) == (mode == "band")
    (cb, fb), (cd, fd) = res["band"][:2], res["dense"][:2]
    assert np.isfinite(cb) and abs(cb - cd) <= 1e-4, (cb, cd)
    assert np.allclose(np.asarray(fb, dtype=np.float64), np.asarray(fd, dtype=np.float64), rtol=0, atol=1e-3), (fb, fd)
    REPORT.append({"case": "trainer_test_eval_tail_long", "corr_band": float(cb), "corr_dense": float(cd), "f_band": [float(v) for v in np.ravel(fb)],
                   "f_dense": [float(v) for v in np.ravel(fd)], "band_calls": len(calls)})
    print("Trainer.test band / dense: corr", cb, cd, "F", fb, fd, "band scoring calls (rows)", calls)


# ------------------------------------------------------------------------------------------------ 5. offsets past 2^31 bytes
def test_offsets_past_2_31_bytes(dev):
    """One video of 262 144 steps, D = 64, w = 1024: 4096 strips of 64 x 2112 floats = 2.2 GB of logits, so byte offsets into the band pass
    2^31 (element offsets times 4).  Checked on 3 x 64 rows: the first strip, the strip that holds byte 2^31 of the band, the last strip."""
    T, D, w = 262144, 64, 1024
    gen = torch.Generator(device=dev); gen.manual_seed(262144)
    x = torch.randn(T, 3 * D, generator=gen, device=dev)
    q, k, v = x[:, :D], x[:, D:2 * D], x[:, 2 * D:]
    rc, ctx, _, need = _raw(dev, q, k, v, [T], w, 0.125, False)
    assert rc == 0 and need > 2 ** 31
    pitch = 2 * w + 64
    mid = (2 ** 31) // (64 * pitch * 4)
    assert 0 < mid < T // 64 - 1
    rows = np.concatenate([np.arange(64), 64 * mid + np.arange(64), T - 64 + np.arange(64)])
    xh = x.cpu().numpy()
    c64, _ = attn_band_ref.band_attention(xh[:, :D], xh[:, D:2 * D], xh[:, 2 * D:], [T], w, 0.125, False, rows=rows)
    c32, _ = attn_band_ref.band_attention(xh[:, :D], xh[:, D:2 * D], xh[:, 2 * D:], [T], w, 0.125, False, dtype=np.float32, rows=rows)
    yard, gate = _gate(c64, c32)
    got = ctx[torch.from_numpy(rows).to(dev)].cpu().numpy()
    err = float(np.abs(got - c64).max())
    REPORT.append({"case": "offsets_T262144", "workspace_bytes": need, "strip_with_byte_2_31": int(mid), "error": err, "yardstick": yard, "gate": gate})
    print("attn_band T 262144 workspace", need, "strip", int(mid), "err / yardstick / gate", err, yard, gate)
    assert not np.isnan(got).any() and err <= gate, (err, gate)
    assert not torch.isnan(ctx).any()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_bad_arguments_are_refused(dev):
    from summarizer_amd import _lib, kernels
    from summarizer_amd._lib import SumkError
    lib = _lib.load()
    D, w, lens = 64, 8, [33, 70]
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((sum(lens), 3 * D)).astype(np.float32)).to(dev)
    q, k, v = x[:, :D], x[:, D:2 * D], x[:, 2 * D:]
    rc, want, _, need = _raw(dev, q, k, v, lens, w, 0.125, False)
    assert rc == 0 and not torch.isnan(want).any()
    untouched = lambda t: bool((t.view(torch.uint8) == 255).all())
    x6 = torch.zeros(sum(lens), 6, device=dev)
    bad = [("aperture<0", dict(w=-1), -1), ("D=6", dict(src=x6), -1), ("short workspace", dict(ws_bytes=need - 1), -2),
           ("T too long", dict(lens=[1048577], ws_bytes=4096), -1)]
    for tag, kw, code in bad:
        kw = dict(kw)
        src = kw.pop("src", None)
        qq, kk, vv = (src, src, src) if src is not None else (q, k, v)
        if kw.pop("w", w) < 0:
            rc, ctx, _, _ = _raw_negative(dev, q, k, v, lens)
        else:
            rc, ctx, _, _ = _raw(dev, qq, kk, vv, kw.pop("lens", lens), w, 0.125, False, **kw)
        msg = lib.sumk_last_error().decode()
        assert rc == code and "attn_band" in msg and len(msg) > 15, (tag, rc, msg)
        assert untouched(ctx), tag                                              # nothing was launched
    # the forward: its own limits, scores untouched
    from summarizer_amd.models.vasnet import VASNet
    m = VASNet(input_size=D, attention_aperture=w, local_attention="band").eval().to(dev)
    sb = kernels.SeqBatch.get(lens, dev)
    feats = x[:, :D].contiguous()
    o = m._opts(False)
    good = kernels.vasnet_forward_band(feats, sb, m._params(), o)
    assert torch.isfinite(good).all()
    for tag, change, word in [("no aperture", dict(aperture=None), "aperture"), ("bf16x6", dict(precision="bf16x6"), "fp32"),
                              ("dropout", dict(dropout_p=0.5), "dropout")]:
        with pytest.raises(SumkError, match=word):
            kernels.vasnet_forward_band(feats, sb, m._params(), dict(o, **change))
    wts, so = kernels._vasnet_structs(m._params(), dict(o))
    scores = torch.full((sum(lens),), float("nan"), device=dev); scores.view(torch.uint8).fill_(255)
    nb = kernels.vasnet_band_workspace_bytes(D, sb, w)
    ws = torch.full((nb,), 255, dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.sumk_vasnet_forward_band(feats.data_ptr(), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(wts), C.byref(so), scores.data_ptr(),
                                      ws.data_ptr(), nb - 1, st)
    torch.cuda.synchronize()
    assert rc == -2 and "workspace" in lib.sumk_last_error().decode() and untouched(scores)
    rc = lib.sumk_vasnet_forward_band(feats.data_ptr(), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(wts), C.byref(so), scores.data_ptr(),
                                      ws.data_ptr(), nb, st)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(scores.view(torch.int32), good.view(torch.int32))      # and a good call after the refusals
    REPORT.append({"case": "refusals", "refused": len(bad) + 4, "mismatches": 0})


def _raw_negative(dev, q, k, v, lens):
    """sumk_attn_band with aperture = -1 (the workspace query refuses it too: a small made-up workspace)."""
    from summarizer_amd import _lib
    lib = _lib.load()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    off_dev = torch.from_numpy(off).to(dev)
    ws = torch.full((4096,), 255, dtype=torch.uint8, device=dev)
    ctx = torch.empty(q.shape[0], q.shape[1], device=dev); ctx.view(torch.uint8).fill_(255)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.sumk_attn_band(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), q.shape[1], len(lens), _lib.host_i32(off),
                            off_dev.data_ptr(), 0.125, 0, -1, ctx.data_ptr(), ctx.stride(0), None, ws.data_ptr(), 4096, st)
    torch.cuda.synchronize()
    return rc, ctx, None, 0
