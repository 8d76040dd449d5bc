"""GPU: TRAINING on the band (csrc/attn_band_bwd.hip: sumk_attn_band_forward_train / _backward, sumk_vasnet_forward_band_train /
_backward_band), kernels.attn_band_train / attn_band_backward, VASNet(local_attention_train="band") and VASNetTrainer on it.

Gates
  * kernel level: dQ, dK, dV against the float64 band-only specification tests/attn_band_bwd_ref.py (pinned to torch.autograd on the dense
    formula in tests/test_attn_band_bwd_host.py): per case and tensor max |hip - f64| <= max(4 x max |spec_f32 - f64|, 2 x 2^-23 x max |f64|),
    the project's standing gate; the float32 run sums every product as one accumulator chain (tests/attn_band_ref.py says why).  Dropout
    masks of the specification come from recipes.dropout_keep at site 0, index (packed_row << 20) | key.
  * model level: every parameter gradient and dx within 3e-4 of the tensor's largest magnitude (the project's gradient parity) of
    autograd through oracle/torch_port.vasnet_scores at float64 with recipes.vasnet_drop_masks of the kernel's seed.
Every test prints its figures and keeps them in REPORT (written to $SUMK_REPORT_DIR/attn_band_bwd.json when set).

Measured on MI355X (worst over the 72 cases of test 1): error / yardstick dQ 1.45, dK 1.50, dV 1.51 (limit 4); offsets past 2^31 bytes
(T = 1 048 576): errors 2.0e-7 .. 3.9e-7, yardsticks 2.1e-7 .. 7.6e-7; model gradients at most 4.2e-6 of the tensor's largest magnitude from
float64 (gate 3e-4) and at most 3.4e-6 from the dense path; trainer losses 0.199 -> 0.181 over two epochs."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import attn_band_bwd_ref
from oracle import torch_port

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
REPORT = []
LENS = [1, 65, 200, 64, 333, 2]
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
WINDOWS = [0, 1, 31, 32, 63, 64, 100, 332, 5000]
SEED, P = 20261, 0.5
NAMES = ("dQ", "dK", "dV")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for r in REPORT:
        print("ATTN-BAND-BWD-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "attn_band_bwd.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


# ------------------------------------------------------------------------------------------------ inputs, references and calls
@functools.lru_cache(maxsize=None)
def _data(D):
    """(rows, 4 D) float32 [Q | K | V | dCTX] ~ N(0, 1) for LENS, no planted row; read-only."""
    x = np.random.default_rng(5200 + D).standard_normal((sum(LENS), 4 * D)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _keep(w, seed, p):
    """Scaled keep masks of site 0 in band layout (rows x (2 w + 1)) for LENS, indexed as the kernels index them; None at p = 0."""
    import recipes as R
    if p == 0:
        return None
    out = np.zeros((sum(LENS), 2 * w + 1), dtype=np.float32)
    for v, T in enumerate(LENS):
        i = np.arange(T, dtype=np.int64)
        key = np.clip(i[:, None] - w + np.arange(2 * w + 1, dtype=np.int64)[None, :], 0, T - 1)
        idx = ((i[:, None] + OFF[v]).astype(np.uint64) << np.uint64(20)) | key.astype(np.uint64)
        out[OFF[v]:OFF[v] + T] = R.dropout_keep(seed, 0, idx, p).astype(np.float32) * (np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    out.setflags(write=False)
    return out


def _spec_of(x, D, w, ignore_self, keep):
    a = (x[:, :D], x[:, D:2 * D], x[:, 2 * D:3 * D], x[:, 3 * D:])
    out = attn_band_bwd_ref.band_attention_backward(*a, LENS, w, 1.0 / np.sqrt(D), ignore_self, keep=keep)
    out += attn_band_bwd_ref.band_attention_backward(*a, LENS, w, 1.0 / np.sqrt(D), ignore_self, keep=keep, dtype=np.float32)
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _spec(D, w, ignore_self, p, seed=SEED):
    """(dQ64, dK64, dV64, dQ32, dK32, dV32) of the specification -- computed once per case, shared by the tests, never modified."""
    return _spec_of(_data(D), D, w, ignore_self, _keep(w, seed, p))


def _gate(s64, s32):
    fin = ~np.isnan(s64)
    assert np.array_equal(fin, ~np.isnan(s32))
    if not fin.any():
        return 0.0, 0.0
    yard = float(np.abs(s32[fin].astype(np.float64) - s64[fin]).max())
    return yard, max(4 * yard, 2 * EPS * float(np.abs(s64[fin]).max()))


def _split(dev, D, x=None):
    """Q, K, V, dCTX on the device: D = 64 with Q | K | V as column blocks of ONE (rows, 3 D) tensor (leading dimension 3 D) and a dense dCTX,
    otherwise four dense tensors."""
    t = torch.from_numpy(np.array(_data(D) if x is None else x)).to(dev)
    if D == 64:
        qkv = t[:, :3 * D].contiguous()
        return [qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], t[:, 3 * D:].contiguous()]
    return [t[:, k * D:(k + 1) * D].contiguous() for k in range(4)]


def _poisoned(dev, shape, fill, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(fill)
    return t


def _run(dev, q, k, v, dc, lens, w, scale, ignore_self, p=0.0, seed=SEED, seed_dev=None, fill=255, bufs=None):
    """forward-train + backward on buffers of this test, workspace and outputs handed over filled with the byte `fill` (0xFF: NaN).
    Returns (ctx, dq, dk, dv, ws).  bufs: (ws, ctx, dq, dk, dv) to reuse -- a call inside a graph capture allocates nothing."""
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(lens, dev)
    D = q.shape[1]
    if bufs is None:
        ws = _poisoned(dev, (kernels.attn_band_train_workspace_bytes(D, sb, w),), fill, torch.uint8)
        ctx, dq, dk, dv = (_poisoned(dev, (q.shape[0], D), fill) for _ in range(4))
    else:
        ws, ctx, dq, dk, dv = bufs
    kw = dict(ignore_self=ignore_self, dropout_p=p, seed=seed, seed_dev=seed_dev)
    kernels.attn_band_train(q, k, v, sb, w, scale, ctx=ctx, ws=ws, **kw)
    kernels.attn_band_backward(q, k, v, dc, sb, w, scale, ws, out=(dq, dk, dv), **kw)
    if bufs is None:
        torch.cuda.synchronize()
    return ctx, dq, dk, dv, ws


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("w", WINDOWS)
def test_attn_band_backward_against_float64(dev, D, w):
    q, k, v, dc = _split(dev, D)
    for ignore_self in (False, True):
        for p in (0.0, P):
            spec = _spec(D, w, ignore_self, p)
            got = [t.cpu().numpy() for t in _run(dev, q, k, v, dc, LENS, w, 1.0 / np.sqrt(D), ignore_self, p)[1:4]]
            rec = {"case": f"f64_D{D}_w{w}_self{int(ignore_self)}_p{p}"}
            bad = []
            for name, g, s64, s32 in zip(NAMES, got, spec[:3], spec[3:]):
                yard, gate = _gate(s64, s32)
                fin = ~np.isnan(s64)
                err = float(np.abs(g[fin] - s64[fin]).max()) if fin.any() else 0.0
                rec.update({f"{name}_error": err, f"{name}_yardstick": yard, f"{name}_gate": gate, f"{name}_ratio": err / yard if yard > 0 else 0.0})
                if not np.array_equal(np.isnan(g), ~fin) or not err <= gate:
                    bad.append((name, err, yard, gate))
            REPORT.append(rec)
            print("attn_band_bwd", json.dumps(rec))
            assert not bad, bad
            if w == 0 and p == 0 and not ignore_self:                          # one key, weight exactly 1: dV IS dCTX, dQ and dK are exactly 0
                assert np.array_equal(got[2].view(np.int32), dc.cpu().numpy().view(np.int32))
                assert (got[0] == 0).all() and (got[1] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. NaN and isolation
@pytest.mark.parametrize("w", [1, 31, 100])
def test_nan_stays_where_the_band_puts_it(dev, w):
    D, bad = 64, 3
    r0, r1 = int(OFF[bad]), int(OFF[bad + 1])
    clean = [_bits(t) for t in _run(dev, *_split(dev, D), LENS, w, 0.125, False)[1:4]]
    assert not any(np.isnan(c.view(np.float32)).any() for c in clean)
    # (a) one video all NaN: every other video's rows are bit-equal to the clean run
    x = np.array(_data(D)); x[r0:r1] = np.nan
    got = [_bits(t) for t in _run(dev, *_split(dev, D, x), LENS, w, 0.125, False)[1:4]]
    other = np.ones(sum(LENS), dtype=bool); other[r0:r1] = False
    for name, g, c in zip(NAMES, got, clean):
        assert np.isnan(g.view(np.float32)[r0:r1]).all(), name
        assert np.array_equal(g[other], c[other]), name
    # (b) an all-zero query row = an all-masked row: dQ row NaN, dK / dV NaN exactly at the keys of its band (the specification's positions)
    zr = int(OFF[4]) + 100
    x = np.array(_data(D)); x[zr, :D] = 0.0
    spec = _spec_of(x, D, w, False, None)
    got = [_bits(t) for t in _run(dev, *_split(dev, D, x), LENS, w, 0.125, False)[1:4]]
    other = np.ones(sum(LENS), dtype=bool); other[OFF[4]:OFF[5]] = False
    band = np.zeros(sum(LENS), dtype=bool); band[zr - w:zr + w + 1] = True
    for name, g, c, s64 in zip(NAMES, got, clean, spec[:3]):
        assert np.array_equal(np.isnan(g.view(np.float32)), np.isnan(s64)), name
        assert np.array_equal(np.isnan(s64).all(axis=1), [zr == r for r in range(sum(LENS))] if name == "dQ" else band), name
        assert np.array_equal(g[other], c[other]), name
    REPORT.append({"case": f"nan_isolation_w{w}", "rows_compared": int(other.sum()), "mismatches": 0})


# ------------------------------------------------------------------------------------------------ 3. determinism and capture
def test_deterministic_captures_and_draws_fresh_masks(dev):
    D, w, seed = 64, 40, 991
    q, k, v, dc = _split(dev, D)
    a = _run(dev, q, k, v, dc, LENS, w, 0.125, True, P, seed)
    b = _run(dev, q, k, v, dc, LENS, w, 0.125, True, P, seed, fill=0x5A)
    same = lambda s, t: torch.equal(s.view(torch.int32), t.view(torch.int32))
    assert all(same(s, t) for s, t in zip(a[:4], b[:4]))
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    bufs = (torch.full_like(a[4], 255),) + tuple(torch.zeros_like(t) for t in a[:4])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run(dev, q, k, v, dc, LENS, w, 0.125, True, P, seed, seed_dev=word, bufs=bufs)
    for _ in range(2):
        bufs[0].fill_(255)
        for t in bufs[1:]:
            t.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(same(s, t) for s, t in zip(bufs[1:], a[:4]))
    # the device word moves the seed: other masks, those of seed + word -- the eager run with that seed, which the specification with
    # recipes.dropout_keep(seed + word, ...) describes
    word.add_(1)
    bufs[0].fill_(255)
    g.replay()
    torch.cuda.synchronize()
    c = _run(dev, q, k, v, dc, LENS, w, 0.125, True, P, seed + 1)
    assert all(same(s, t) for s, t in zip(bufs[1:], c[:4])) and not same(bufs[4], a[3])
    spec = _spec(D, w, True, P, seed + 1)
    for name, t, s64, s32 in zip(NAMES, bufs[2:], spec[:3], spec[3:]):
        yard, gate = _gate(s64, s32)
        got, fin = t.cpu().numpy(), ~np.isnan(s64)                            # (ignore_self: the one-step video's row is all-masked)
        assert np.array_equal(np.isnan(got), ~fin), name
        err = float(np.abs(got[fin] - s64[fin]).max())
        print("replay with seed word 1:", name, "err / yardstick / gate", err, yard, gate)
        assert err <= gate, (name, err, gate)
    REPORT.append({"case": "determinism_capture_seed_word", "replays": 3, "mismatches": 0})


# ------------------------------------------------------------------------------------------------ 4. offsets past 2^31 bytes
def test_offsets_past_2_31_bytes(dev):
    """One video of 1 048 576 steps, D = 64, w = 256: 16 384 strips of 64 x 576 floats = 2.4 GB per rectangle buffer, so byte offsets into E, E2
    and ET pass 2^31.  Checked on 3 x 64 rows / keys: the first strip, the strip that holds byte 2^31 of a buffer, the last strip.  The
    specification runs on the window of rows within 2 w of each checked strip: every row that sees a checked key has all its keys there."""
    T, D, w = 1048576, 64, 256
    gen = torch.Generator(device=dev); gen.manual_seed(1048576)
    x = torch.randn(T, 4 * D, generator=gen, device=dev)
    q, k, v, dc = (x[:, i * D:(i + 1) * D] for i in range(4))
    _, dq, dk, dv, ws = _run(dev, q, k, v, dc, [T], w, 0.125, False)
    assert ws.numel() > 3 * 2 ** 31
    mid = (2 ** 31) // (64 * (2 * w + 64) * 4)
    assert 0 < mid < T // 64 - 1
    rec = {"case": "offsets_T1048576", "workspace_bytes": int(ws.numel()), "strip_with_byte_2_31": int(mid)}
    for s0 in (0, 64 * mid, T - 64):
        lo, hi = max(0, s0 - 2 * w), min(T, s0 + 64 + 2 * w)
        xh = x[lo:hi].cpu().numpy()
        a = [xh[:, i * D:(i + 1) * D] for i in range(4)]
        s64 = attn_band_bwd_ref.band_attention_backward(*a, [hi - lo], w, 0.125, False)
        s32 = attn_band_bwd_ref.band_attention_backward(*a, [hi - lo], w, 0.125, False, dtype=np.float32)
        sl = slice(s0 - lo, s0 - lo + 64)
        for name, t, r64, r32 in zip(NAMES, (dq, dk, dv), s64, s32):
            yard, gate = _gate(r64[sl], r32[sl])
            err = float(np.abs(t[s0:s0 + 64].cpu().numpy() - r64[sl]).max())
            rec[f"{name}_row{s0}"] = [err, yard, gate]
            assert err <= gate, (name, s0, err, gate)
    for t in (dq, dk, dv):
        assert not torch.isnan(t).any()
    REPORT.append(rec)
    print("attn_band_bwd offsets", json.dumps(rec))


# ------------------------------------------------------------------------------------------------ 5. model level
MODEL_LENS = [1, 65, 300, 129]


def _models(dev, D, w, **kw):
    from summarizer_amd.models.vasnet import VASNet
    torch.manual_seed(100 + D + w)
    band = VASNet(input_size=D, attention_aperture=w, local_attention="band", local_attention_train="band", **kw).train()
    dense = VASNet(input_size=D, attention_aperture=w, **kw).train()
    dense.load_state_dict(band.state_dict())
    return band.to(dev), dense.to(dev)


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _model_case(dev, D, w, tag, **kw):
    import recipes as R
    band, dense = _models(dev, D, w, **kw)
    xs = [R.features(T, 1, D, 70 + T) - 0.1 for T in MODEL_LENS]
    cw = np.random.default_rng(6).standard_normal(sum(MODEL_LENS)).astype(np.float32)
    xh = np.concatenate([a[:, 0] for a in xs])
    grads = {}
    for name, m in (("band", band), ("dense", dense)):
        torch.manual_seed(77)
        m._seed_counter = 0
        x = torch.from_numpy(xh).to(dev).requires_grad_(True)
        s = m.score_packed(x, MODEL_LENS)
        (s * torch.from_numpy(cw).to(dev)).sum().backward()
        grads[name] = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
        grads[name]["x"] = x.grad.cpu().numpy()
        grads[name]["scores"] = s.detach().cpu().numpy()
    seed = (torch.initial_seed() * 1000003 + band._seed_counter) & (2 ** 63 - 1)         # VASNet._opts
    masks = R.vasnet_drop_masks(seed, float(band.dropout.p), MODEL_LENS, D)
    pt = {k: p.detach().cpu().double().requires_grad_(True) for k, p in band.named_parameters()}
    table = pt.get("pos_embed.weight")
    ref_x, ref_s, r0 = [], [], 0
    for a, dm in zip(xs, masks):
        xt = torch.from_numpy(a).double().requires_grad_(True)
        sc = torch_port.vasnet_scores(xt, pt, aperture=w, pos_table=table, drop_masks=tuple(torch.from_numpy(t).double().unsqueeze(0) for t in dm))
        (sc.reshape(-1) * torch.from_numpy(cw[r0:r0 + a.shape[0]]).double()).sum().backward()
        ref_x.append(xt.grad.numpy()[:, 0]); ref_s.append(sc.detach().reshape(-1).numpy()); r0 += a.shape[0]
    ref = {k: t.grad.numpy() for k, t in pt.items()}
    ref["x"] = np.concatenate(ref_x)
    assert float(np.abs(grads["band"]["scores"] - np.concatenate(ref_s)).max()) <= 1e-4
    rec = {"case": f"model_{tag}_D{D}_w{w}"}
    worst = {}
    for key, r in ref.items():
        worst[key] = _rel(grads["band"][key], r)
        rec[key] = {"error_vs_f64": worst[key], "distance_to_dense_path": _rel(grads["band"][key], grads["dense"][key])}
    REPORT.append(rec)
    print("band training", json.dumps(rec))
    assert all(np.isfinite(grads["band"][key]).all() for key in ref)
    assert max(worst.values()) <= 3e-4, worst
    return rec


@pytest.mark.parametrize("D,w", [(64, 0), (64, 16), (64, 64), (1024, 16)])
def test_band_training_gradients_against_float64(dev, D, w):
    _model_case(dev, D, w, "plain")


def test_band_training_with_positions(dev):
    rec = _model_case(dev, 64, 16, "positions", max_length=512)
    assert "pos_embed.weight" in rec


def test_forward_with_a_positional_table_is_refused(dev):
    from summarizer_amd._lib import SumkError
    band, _ = _models(dev, 64, 16, max_length=512)
    with pytest.raises(SumkError, match="score_packed"):
        band(torch.zeros(40, 1, 64, device=dev))


# ------------------------------------------------------------------------------------------------ 6. trainer
def test_trainer_trains_on_the_band(dev, monkeypatch):
    from summarizer_amd import kernels
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.datasets import synthetic_dataset
    from summarizer_amd.utils.hps import make_hps
    ds = synthetic_dataset(8, seed=5, D=64, t_range=(40, 90), n_users=4)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
    hps = make_hps(ds, [{"train_keys": keys[2:], "test_keys": keys[:2]}], epochs=2, test_every_epochs=1, lr=1e-3,
                   extra_params={"input_size": "64", "local": "16", "local_attention": "band", "local_attention_train": "band"})

    def no_dense(*a, **k):
        raise AssertionError("the dense path was asked for a workspace")
    monkeypatch.setattr(kernels, "vasnet_forward_packed", no_dense)
    calls = []
    real = kernels.vasnet_backward_band
    monkeypatch.setattr(kernels, "vasnet_backward_band", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(3); random.seed(3)
    tr = VASNetTrainer(hps, hps.splits_files[0]).reset()
    assert tr.model.local_attention_train == "band"
    best = tr.train(0)
    losses = [v for _, v in hps.writer.scalars["synthetic/Fold_1/Train/Loss"]]
    print("trainer on the band: losses", losses, "best", best, "band backward calls", len(calls))
    assert len(calls) == 2 * (len(keys) - 2)                                    # every step eager, every step on the band
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[1] < losses[0], losses
    assert all(np.isfinite(best))
    REPORT.append({"case": "trainer_two_epochs", "losses": [float(v) for v in losses], "band_backward_calls": len(calls)})


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_bad_arguments_are_refused(dev):
    from summarizer_amd import _lib, kernels
    from summarizer_amd._lib import SumkError
    from summarizer_amd.models.vasnet import VASNet
    lib = _lib.load()
    D, w, lens = 64, 8, [33, 70]
    sb = kernels.SeqBatch.get(lens, dev)
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((sum(lens), 4 * D)).astype(np.float32)).to(dev)
    q, k, v, dc = (x[:, i * D:(i + 1) * D] for i in range(4))
    untouched = lambda *ts: all(bool((t.view(torch.uint8) == 255).all()) for t in ts)
    need = kernels.attn_band_train_workspace_bytes(D, sb, w)
    ws = _poisoned(dev, (need,), 255, torch.uint8)
    out = [_poisoned(dev, (sum(lens), D), 255) for _ in range(4)]
    for tag, kw, word in [("p=1", dict(dropout_p=1.0), "dropout_p"), ("p<0", dict(dropout_p=-0.5), "dropout_p"), ("short workspace", dict(ws=ws[:need - 256]), "workspace")]:
        kw = dict(kw)
        wsk = kw.pop("ws", ws)
        with pytest.raises(SumkError, match=word):
            kernels.attn_band_train(q, k, v, sb, w, 0.125, ctx=out[0], ws=wsk, **kw)
        with pytest.raises(SumkError, match=word):
            kernels.attn_band_backward(q, k, v, dc, sb, w, 0.125, wsk, out=tuple(out[1:]), **kw)
        torch.cuda.synchronize()
        assert untouched(ws, *out), tag                                         # nothing was launched
    with pytest.raises(SumkError, match="aperture"):
        kernels.attn_band_train(q, k, v, sb, -1, 0.125, ctx=out[0], ws=ws)
    # the model: constructor and call refusals
    with pytest.raises(SumkError, match="local_attention_train"):
        VASNet(input_size=D, attention_aperture=w, local_attention_train="band")
    with pytest.raises(SumkError, match="fp32"):
        VASNet(input_size=D, attention_aperture=w, local_attention="band", local_attention_train="band", precision="bf16")
    with pytest.raises(SumkError, match="fold_vo"):
        VASNet(input_size=D, attention_aperture=w, local_attention="band", local_attention_train="band", fold_vo=True)
    # the VASNet pair: its own limits, scores and gradients untouched
    m = VASNet(input_size=D, attention_aperture=w, local_attention="band", local_attention_train="band").train().to(dev)
    feats = x[:, :D].contiguous()
    o = dict(m._opts(True))
    nb = kernels.vasnet_band_train_workspace_bytes(D, sb, w)
    vws = _poisoned(dev, (nb,), 255, torch.uint8)
    grads = {kk: _poisoned(dev, tuple(p.shape), 255) for kk, p in m.named_parameters()}
    dscores = torch.ones(sum(lens), device=dev)
    for tag, change, word in [("no aperture", dict(aperture=None), "aperture"), ("bf16x6", dict(precision="bf16x6"), "fp32"), ("bf16", dict(precision="bf16"), "fp32"),
                              ("p=1", dict(dropout_p=1.0), "dropout_p")]:
        with pytest.raises(SumkError, match=word):
            kernels.vasnet_forward_band_train(feats, sb, m._params(), dict(o, **change), ws=vws)
        with pytest.raises(SumkError, match=word):
            kernels.vasnet_backward_band(feats, sb, m._params(), dict(o, **change), dscores, vws, grads)
    with pytest.raises(SumkError, match="workspace"):
        kernels.vasnet_forward_band_train(feats, sb, m._params(), o, ws=vws[:nb - 256])
    with pytest.raises(SumkError, match="workspace"):
        kernels.vasnet_backward_band(feats, sb, m._params(), o, dscores, vws[:nb - 256], grads)
    torch.cuda.synchronize()
    assert untouched(vws, *grads.values())
    # and a good step after the refusals
    scores, _ = kernels.vasnet_forward_band_train(feats, sb, m._params(), o, ws=vws)
    for t in grads.values():
        t.zero_()
    kernels.vasnet_backward_band(feats, sb, m._params(), o, dscores, vws, grads)
    torch.cuda.synchronize()
    assert torch.isfinite(scores).all() and all(torch.isfinite(t).all() and float(t.abs().max()) > 0 for t in grads.values())
    assert lib.sumk_last_error() is not None
    REPORT.append({"case": "refusals", "refused": 26, "mismatches": 0})
