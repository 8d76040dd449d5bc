"""CPU: the pieces of TRAINING on the band that need no GPU -- the O(T w) backward specification tests/attn_band_bwd_ref.py pinned against
torch.autograd on the dense float64 formula of oracle/torch_port.vasnet_scores (logits, mask, softmax, mask multiply, bmm), the two
training workspace queries against a restatement of their formula, and the constructor checks of VASNet(local_attention_train=...)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import attn_band_bwd_ref
from conftest import ROOT

LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")
D = 16


def _inputs(T, seed=0):
    rng = np.random.default_rng(1700 + T + seed)
    return tuple(rng.standard_normal((T, D)).astype(np.float32).astype(np.float64) for _ in range(4))      # Q, K, V, dCTX; no zero row


def _dense_autograd(Q, K, V, dC, w, scale, ignore_self, keep_dense):
    """dQ, dK, dV of ctx = (softmax(mask(Q K^T * scale)) * keep) V by torch.autograd at float64: torch_port.vasnet_scores lines 77-86."""
    q, k, v = (torch.from_numpy(a).clone().requires_grad_(True) for a in (Q, K, V))
    T = Q.shape[0]
    e = torch.bmm(q[None], k[None].transpose(1, 2)) * scale
    if ignore_self:
        e = e.masked_fill(torch.eye(T, dtype=torch.bool).unsqueeze(0), float("-inf"))
    scope = torch.tril(e, diagonal=w) * torch.triu(e, diagonal=-w)
    e = e.masked_fill(scope == 0, float("-inf"))
    alpha = torch.softmax(e, dim=2)
    if keep_dense is not None:
        alpha = alpha * torch.from_numpy(keep_dense)[None]
    c = torch.bmm(alpha, v[None])
    c.backward(torch.from_numpy(dC)[None])
    return q.grad.numpy(), k.grad.numpy(), v.grad.numpy()


def _band_keep(keep_dense, w):
    """dense (T, T) keep mask -> band layout (T, 2 w + 1); columns of keys outside the video hold a value the spec must ignore."""
    T = keep_dense.shape[0]
    out = np.full((T, 2 * w + 1), 77.0)
    for i in range(T):
        lo, hi = max(0, i - w), min(T, i + w + 1)
        out[i, lo - (i - w):hi - (i - w)] = keep_dense[i, lo:hi]
    return out


@pytest.mark.parametrize("ignore_self", [False, True])
@pytest.mark.parametrize("w", [0, 1, 31, 64, 5000])
@pytest.mark.parametrize("T", [1, 2, 65, 200])
def test_backward_spec_equals_dense_autograd(T, w, ignore_self):
    """Same formula, other summation order: the float64 runs agree within 1e-12 (|values| < 40, at most 200 terms -> rounding ~1e-13).  The
    inputs have no all-masked row except where the case itself masks EVERY row (ignore_self with one key per row: T = 1 or w = 0).  There
    the two sides are different definitions, on purpose: alpha is NaN, so dV is NaN on both sides; autograd's masked_fill hands a masked
    logit the gradient 0, so torch's dQ / dK are 0, while the kernels (dense and band: dLogits = scale * alpha * (...), alpha = NaN) and
    this specification give NaN.  Those cases check exactly that."""
    Q, K, V, dC = _inputs(T)
    scale = 1.0 / np.sqrt(D)
    keep_dense = (np.random.default_rng(T * 31 + w).random((T, T)) >= 0.5) * 2.0
    all_masked = ignore_self and (T == 1 or w == 0)
    for kd in (None, keep_dense):
        want = _dense_autograd(Q, K, V, dC, w, scale, ignore_self, kd)
        got = attn_band_bwd_ref.band_attention_backward(Q, K, V, dC, [T], w, scale, ignore_self, keep=None if kd is None else _band_keep(kd, w))
        for name, a, b in zip(("dQ", "dK", "dV"), got, want):
            assert a.shape == (T, D) and a.dtype == np.float64
            if all_masked:           # (one key per row, the diagonal; a dropped weight is 0 in the specification -- the kernels select -- and NaN x 0 in torch)
                kept = np.ones(T, dtype=bool) if kd is None or name != "dV" else kd.diagonal() != 0
                assert np.array_equal(np.isnan(a).all(axis=1), kept) and np.array_equal(np.isnan(a).any(axis=1), kept), (name, T, w)
                assert np.isnan(b).all() if name == "dV" else (b == 0).all(), (name, T, w)
                continue
            assert not np.isnan(a).any() and not np.isnan(b).any(), (name, T, w)
            assert float(np.abs(a - b).max()) <= 1e-12, (name, T, w, float(np.abs(a - b).max()))


def test_backward_spec_packed_batch_nan_row_and_chain():
    """Videos of a packed batch are independent; an all-masked (zero) query row gives a NaN dQ row and NaN in dK / dV at the keys of its band
    only; the one-accumulator chain of the float32 yardstick is the same formula (1e-12 at float64) and the float32 run has its NaN positions."""
    lens, w = [1, 65, 200, 2], 7
    parts = [_inputs(T, seed=3) for T in lens]
    Q, K, V, dC = (np.concatenate([p[k] for p in parts]) for k in range(4))
    zr = 1 + 65 + 100
    Q[zr] = 0.0
    keep = (np.random.default_rng(5).random((sum(lens), 2 * w + 1)) >= 0.5) * 2.0
    got = attn_band_bwd_ref.band_attention_backward(Q, K, V, dC, lens, w, 0.25, True, keep=keep)
    r0 = 0
    for T in lens:
        sl = slice(r0, r0 + T)
        one = attn_band_bwd_ref.band_attention_backward(Q[sl], K[sl], V[sl], dC[sl], [T], w, 0.25, True, keep=keep[sl])
        assert all(np.array_equal(a[sl], b, equal_nan=True) for a, b in zip(got, one))
        r0 += T
    plain = attn_band_bwd_ref.band_attention_backward(Q, K, V, dC, lens, w, 0.25, False)
    nan_q = np.zeros(sum(lens), dtype=bool); nan_q[zr] = True
    nan_k = np.zeros(sum(lens), dtype=bool); nan_k[zr - w:zr + w + 1] = True
    for a, rows in zip(plain, (nan_q, nan_k, nan_k)):
        assert np.array_equal(np.isnan(a).any(axis=1), rows) and np.array_equal(np.isnan(a).all(axis=1), rows)
    chained = attn_band_bwd_ref.band_attention_backward(Q, K, V, dC, lens, w, 0.25, False, chain=True)
    f32 = attn_band_bwd_ref.band_attention_backward(Q, K, V, dC, lens, w, 0.25, False, dtype=np.float32)
    for a, b, c in zip(plain, chained, f32):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(a), np.isnan(c)) and c.dtype == np.float32
        assert float(np.abs(np.nan_to_num(a) - np.nan_to_num(b)).max()) <= 1e-12
        assert float(np.abs(np.nan_to_num(a) - np.nan_to_num(c)).max()) <= 1e-4


# ------------------------------------------------------------------------------------------------ the C entries, without a device
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    from summarizer_amd import _lib
    return _lib.load()


def _off(lens):
    return (C.c_int32 * (len(lens) + 1))(*np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist())


def _al(n):
    return (n + 255) // 256 * 256


def _band_bytes(lens, w, n_e, n_tab):
    """The band's layout restated: n_e rectangle buffers, one 32-byte record per video and per strip, n_tab tables of 96 bytes per strip."""
    w = min(w, 1048576)
    e = strips = 0
    for T in lens:
        s = (T + 63) // 64
        pitch = (min(T, 2 * w + 64) + 3) // 4 * 4
        e += s * 64 * pitch; strips += s
    return n_e * _al(4 * e) + _al(32 * len(lens)) + _al(32 * strips) + n_tab * _al(96 * strips)


def _vasnet_train_bytes(D_, lens, w):
    R = sum(lens)
    rd = _al(4 * R * D_)
    acts = 8 * rd + 2 * _al(4 * R * 3 * D_)                 # ctx, y0, y1, z, dz, dy1, dy0, dctx; [Q | K | V] and its gradient
    small = _al(16 * R) + _al(4 * R) + _al(768 * (4 * D_ + 4) * 4) + _al(4 * 32 * D_ * D_) + _al(2 * 64 * 96) + _al(3 * 96)
    return acts + small + _band_bytes(lens, w, 3, 6)


def test_training_workspace_queries(lib):
    band = lambda D_, lens, w: lib.sumk_attn_band_train_workspace_bytes(D_, len(lens), _off(lens), w)
    step = lambda D_, lens, w: lib.sumk_vasnet_band_train_workspace_bytes(D_, len(lens), _off(lens), w)
    for q in (band, step):
        for bad in ((64, [130], -1), (6, [130], 8), (0, [130], 8), (64, [130, 0], 8), (64, [1048577], 8)):
            assert q(*bad) == 0, bad
        assert q(64, [1], 0) > 0 and q(64, [1, 2, 65], 2 ** 31 - 1) > 0
        assert q(64, [300], 299) == q(64, [300], 100000) == q(64, [300], 2 ** 31 - 1)
    assert band(64, [], 8) == 0 and lib.sumk_attn_band_train_workspace_bytes(64, 1, None, 8) == 0
    assert step(4096, [130], 8) == 0                                             # the LayerNorm backward's limit, D <= 2048
    for D_, lens, w in ((64, [1, 65, 200, 64, 333, 2], 31), (64, [333], 0), (256, [5000], 256), (1024, [65536], 256), (64, [300], 5000),
                        (64, [1048576], 8)):
        assert band(D_, lens, w) == _band_bytes(lens, w, 3, 6), (D_, lens, w)
        assert step(D_, lens, w) == _vasnet_train_bytes(D_, lens, w), (D_, lens, w)
        assert lib.sumk_attn_band_workspace_bytes(D_, len(lens), _off(lens), w) == _band_bytes(lens, w, 1, 2)      # the scoring layout, unchanged
    # one 65 536-step video at D = 1024, w = 256: a training step fits 5 GiB; the dense path's two logits blocks alone are 32 GiB
    assert step(1024, [65536], 256) < 5 * 2 ** 30
    assert lib.sumk_vasnet_workspace_bytes(1024, 1, _off([65536]), 1) >= 2 ** 35


def test_training_refusals_launch_nothing(lib):
    """Every refused call returns its code with a message before it touches its pointers: these are made up."""
    from summarizer_amd import _lib
    fake = lambda k: C.c_void_p(0x1000 * (k + 1))
    need = lib.sumk_attn_band_train_workspace_bytes(64, 1, _off([33]), 4)

    def fwd(D_=64, w=4, p=0.5, ws_bytes=need, q=fake(0), ld=64):
        return lib.sumk_attn_band_forward_train(q, ld, fake(1), 64, fake(2), 64, D_, 1, _off([33]), fake(4), 0.125, 0, w, p, 7, None, fake(3), 64, fake(5),
                                                ws_bytes, None)

    def bwd(D_=64, w=4, p=0.5, ws_bytes=need, q=fake(0), ld=64):
        return lib.sumk_attn_band_backward(q, ld, fake(1), 64, fake(2), 64, fake(6), 64, D_, 1, _off([33]), fake(4), 0.125, 0, w, p, 7, None, fake(7), 64,
                                           fake(8), 64, fake(9), 64, fake(5), ws_bytes, None)

    for f, name in ((fwd, "attn_band_forward_train"), (bwd, "attn_band_backward")):
        for tag, kw, code, word in [("aperture<0", dict(w=-1), -1, "aperture"), ("D=6", dict(D_=6), -1, "D=6"), ("p=1", dict(p=1.0), -1, "dropout_p"),
                                    ("p<0", dict(p=-0.1), -1, "dropout_p"), ("short workspace", dict(ws_bytes=need - 1), -2, "workspace"),
                                    ("null q", dict(q=None), -1, "null"), ("ldq < D", dict(ld=60), -1, "leading")]:
            rc = f(**kw)
            msg = lib.sumk_last_error().decode()
            assert rc == code and name in msg and word in msg, (name, tag, rc, msg)

    wts = _lib.VasnetWeights(*[0x2000 * (k + 1) for k in range(10)])
    grads = _lib.VasnetGrads(*[0x4000 * (k + 1) for k in range(10)])
    need = lib.sumk_vasnet_band_train_workspace_bytes(64, 1, _off([33]), 4)

    def opts(w, precision, p):
        return _lib.VasnetOpts(0.125, 1e-6, 0, w, p, 0, precision, None, None, None, None, None)

    def vf(w=4, precision=0, p=0.5, ws_bytes=need, x=fake(0)):
        return lib.sumk_vasnet_forward_band_train(x, 64, 1, _off([33]), fake(1), C.byref(wts), C.byref(opts(w, precision, p)), fake(2), fake(3), ws_bytes, None)

    def vb(w=4, precision=0, p=0.5, ws_bytes=need, x=fake(0)):
        return lib.sumk_vasnet_backward_band(x, 64, 1, _off([33]), fake(1), C.byref(wts), C.byref(opts(w, precision, p)), fake(2), C.byref(grads), None,
                                             fake(3), ws_bytes, None, None)

    for f, name in ((vf, "vasnet_forward_band_train"), (vb, "vasnet_backward_band")):
        for tag, kw, code, word in [("global attention", dict(w=-1), -1, "aperture"), ("bf16x6", dict(precision=2), -1, "fp32"), ("bf16", dict(precision=3), -1, "fp32"),
                                    ("p=1", dict(p=1.0), -1, "dropout_p"), ("short workspace", dict(ws_bytes=need - 1), -2, "workspace"), ("null x", dict(x=None), -1, "null")]:
            rc = f(**kw)
            msg = lib.sumk_last_error().decode()
            assert rc == code and name in msg and word in msg, (name, tag, rc, msg)


def test_model_constructor_checks():
    from summarizer_amd._lib import SumkError
    from summarizer_amd.models.vasnet import VASNet, VASNetTrainer
    for kw in (dict(local_attention_train="band"), dict(local_attention_train="band", attention_aperture=8),
               dict(local_attention_train="band", attention_aperture=8, local_attention="dense"), dict(local_attention_train="banded", attention_aperture=8)):
        with pytest.raises(SumkError, match="local_attention_train"):
            VASNet(input_size=64, **kw)
    for kw in (dict(precision="bf16"), dict(fold_vo=True)):
        with pytest.raises(SumkError, match="band"):
            VASNet(input_size=64, attention_aperture=8, local_attention="band", local_attention_train="band", **kw)
    m = VASNet(input_size=64, attention_aperture=8, local_attention="band", local_attention_train="band")
    d = VASNet(input_size=64, attention_aperture=8, local_attention="band")
    assert m.local_attention_train == "band" and d.local_attention_train == "dense" and VASNet(input_size=64).local_attention_train == "dense"
    assert list(m.state_dict()) == list(d.state_dict())

    class _Hps:
        extra_params = {"local": "8", "local_attention": "band", "local_attention_train": "band", "input_size": "64"}
        use_cuda = False
    t = VASNetTrainer.__new__(VASNetTrainer)
    t.hps = _Hps()
    assert t._init_model().local_attention_train == "band"
    _Hps.extra_params = {"local": "8", "local_attention": "band", "input_size": "64"}
    assert t._init_model().local_attention_train == "dense"
