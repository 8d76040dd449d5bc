"""CPU: the pieces of local attention on the band that need no GPU -- the O(T w) specification tests/attn_band_ref.py pinned against the dense
oracle (oracle.vasnet_np.attention_mask on the full (T x T) logits, float64), the mask decisions of its float32 run, the workspace queries
(pure host arithmetic), the refusals of the two entry points (made-up pointers, refused calls only) and the constructor checks of
VASNet(local_attention="band")."""
import ctypes as C
import os

import numpy as np
import pytest

import attn_band_ref
from conftest import ROOT
from oracle import vasnet_np

LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")
LENGTHS = (1, 2, 63, 64, 65, 200)
D = 16


def _inputs(T, seed=0):
    rng = np.random.default_rng(900 + T + seed)
    Q, K, V = (rng.standard_normal((T, D)) for _ in range(3))
    Q = Q.astype(np.float32).astype(np.float64); K = K.astype(np.float32).astype(np.float64); V = V.astype(np.float32).astype(np.float64)
    Q[T // 2] = 0.0                                    # one planted all-zero query row: every in-band logit is 0 -> e * e == 0 -> the row is NaN
    return Q, K, V


def _dense(Q, K, V, w, scale, ignore_self):
    """Full (T x T) softmax of the masked logits at float64; alpha cut to the (T x (2 w + 1)) band layout, zeros outside the video."""
    T = Q.shape[0]
    e = vasnet_np.attention_mask((Q @ K.T) * scale, ignore_self, w)
    with np.errstate(invalid="ignore"):
        a = np.exp(e - e.max(axis=1, keepdims=True))
        a = a / a.sum(axis=1, keepdims=True)
        ctx = a @ V
    band = np.zeros((T, 2 * w + 1))
    for i in range(T):
        lo, hi = max(0, i - w), min(T, i + w + 1)
        band[i, lo - (i - w):hi - (i - w)] = a[i, lo:hi]
        out = np.ones(T, dtype=bool); out[lo:hi] = False
        assert np.isnan(a[i]).all() or (a[i, out] == 0).all()      # nothing outside the band carries weight
    return ctx, band


def _windows(T):
    return sorted({0, 1, 31, 64, max(T - 1, 0), T + 7})


@pytest.mark.parametrize("ignore_self", [False, True])
@pytest.mark.parametrize("T", LENGTHS)
def test_band_spec_equals_dense_oracle(T, ignore_self):
    """Same mask decisions, same NaN positions, values within 1e-12: the two differ in the order of the float64 sums only (alpha <= 1,
    |V| < 6, at most 200 terms -> rounding ~1e-14)."""
    Q, K, V = _inputs(T)
    scale = 1.0 / np.sqrt(D)
    for w in _windows(T):
        want_c, want_a = _dense(Q, K, V, w, scale, ignore_self)
        got_c, got_a = attn_band_ref.band_attention(Q, K, V, [T], w, scale, ignore_self)
        assert got_a.shape == (T, 2 * w + 1) and got_c.shape == (T, D)
        assert np.array_equal(np.isnan(want_c), np.isnan(got_c)) and np.array_equal(np.isnan(want_a), np.isnan(got_a)), (T, w)
        assert np.isnan(got_c[T // 2]).all()                                   # the planted row
        if ignore_self and w == 0:
            assert np.isnan(got_c).all()                                       # the only key of every row is the masked diagonal
        fin = ~np.isnan(want_c)
        assert (np.abs(got_c[fin] - want_c[fin]) <= 1e-12).all() and (np.abs(np.nan_to_num(got_a) - np.nan_to_num(want_a)) <= 1e-12).all(), (T, w)
        ok = ~np.isnan(got_a).any(axis=1)
        assert (np.abs(got_a[ok].sum(axis=1) - 1.0) <= 1e-12).all()


def test_band_spec_packed_batch_and_sampled_rows():
    lens = [1, 65, 200, 2]
    parts = [_inputs(T, seed=5) for T in lens]
    Q, K, V = (np.concatenate([p[k] for p in parts]) for k in range(3))
    ctx, alpha = attn_band_ref.band_attention(Q, K, V, lens, 31, 0.25, True)
    r0 = 0
    for T, (q, k, v) in zip(lens, parts):
        c1, a1 = attn_band_ref.band_attention(q, k, v, [T], 31, 0.25, True)
        assert np.array_equal(c1, ctx[r0:r0 + T], equal_nan=True) and np.array_equal(a1, alpha[r0:r0 + T], equal_nan=True)
        r0 += T
    rows = [0, 1, 66, 67, 200, 265, 267]
    cs, als = attn_band_ref.band_attention(Q, K, V, lens, 31, 0.25, True, rows=rows)
    assert np.array_equal(cs, ctx[rows], equal_nan=True) and np.array_equal(als, alpha[rows], equal_nan=True)


@pytest.mark.parametrize("T", LENGTHS)
def test_float32_run_masks_the_same_entries(T):
    """The float32 run of the specification masks what the float64 run masks on these inputs (no in-band logit is so small that its square
    underflows in float32 only), so the GPU tests may compare NaN positions exactly and alpha zeros position by position."""
    Q, K, V = _inputs(T)
    for ignore_self in (False, True):
        for w in _windows(T):
            c64, a64 = attn_band_ref.band_attention(Q, K, V, [T], w, 1.0 / np.sqrt(D), ignore_self)
            c32, a32 = attn_band_ref.band_attention(Q, K, V, [T], w, 1.0 / np.sqrt(D), ignore_self, dtype=np.float32)
            assert c32.dtype == np.float32 and a32.dtype == np.float32
            assert np.array_equal(np.isnan(c64), np.isnan(c32)) and np.array_equal(np.isnan(a64), np.isnan(a32)), (T, w)
            assert np.array_equal(np.nan_to_num(a64) == 0, np.nan_to_num(a32) == 0), (T, w)


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


def test_workspace_queries_need_no_gpu(lib):
    band = lambda D_, lens, w: lib.sumk_attn_band_workspace_bytes(D_, len(lens), _off(lens), w)
    fwd = lambda D_, lens, w: lib.sumk_vasnet_band_workspace_bytes(D_, len(lens), _off(lens), w)
    for q in (band, fwd):
        for bad in ((64, [130], -1), (6, [130], 8), (0, [130], 8), (64, [130, 0], 8), (64, [1048577], 8)):
            assert q(*bad) == 0, bad
        assert q(64, [1048576], 8) > 0 and q(64, [1], 0) > 0 and q(64, [1, 2, 65], 2 ** 31 - 1) > 0
        assert q(64, [300], 299) == q(64, [300], 100000) == q(64, [300], 2 ** 31 - 1)      # the key range is clipped to the video
    assert lib.sumk_attn_band_workspace_bytes(64, 0, _off([]), 8) == 0 and lib.sumk_attn_band_workspace_bytes(64, 1, None, 8) == 0
    # the band: 64-row strips of pitch min(T, 2 w + 64), plus three small tables per strip
    for T, w in ((5000, 256), (65536, 256), (4096, 0), (300, 1000)):
        strips = (T + 63) // 64
        low = strips * 64 * min(T, 2 * w + 64) * 4
        assert low <= band(64, [T], w) <= low + strips * (64 * 16 + 2 * 96 + 32) + 8192, (T, w)
    # one 65 536-step video at D = 1024, w = 256: the whole forward fits 4 GiB, the dense path's logits alone are 16 GiB
    assert 0 < fwd(1024, [65536], 256) < 4 * 2 ** 30
    assert lib.sumk_vasnet_workspace_bytes(1024, 1, _off([65536]), 0) >= 2 ** 34
    # O(T w): doubling T at a fixed w at most doubles the bytes (plus alignment slack)
    for q, D_ in ((band, 64), (fwd, 1024)):
        for T in (4096, 16384, 65536, 524288):
            assert q(D_, [2 * T], 256) <= 2 * q(D_, [T], 256) + 2 ** 20, (D_, T)
            assert q(D_, [T], 512) > q(D_, [T], 256)


def test_refusals_launch_nothing(lib):
    """Every refused call returns its code with a message before it touches its pointers: these are made up."""
    from summarizer_amd import _lib
    fake = lambda k: C.c_void_p(0x1000 * (k + 1))
    need = lib.sumk_attn_band_workspace_bytes(64, 1, _off([33]), 4)

    def band(lens=(33,), D_=64, w=4, ws_bytes=need, q=fake(0), ld=64, ctx=fake(3), ws=fake(5), off_host=True, alpha=None):
        lens = list(lens)
        return lib.sumk_attn_band(q, ld, fake(1), 64, fake(2), 64, D_, len(lens), _off(lens) if off_host else None, fake(4), 0.125, 0, w, ctx, 64,
                                  alpha, ws, ws_bytes, None)

    for tag, kw, code, word in [("aperture<0", dict(w=-1), -1, "aperture"), ("D=6", dict(D_=6), -1, "D=6"), ("T=0", dict(lens=[33, 0]), -1, "steps"),
                                ("T too long", dict(lens=[1048577], ws_bytes=1 << 40), -1, "steps"), ("short workspace", dict(ws_bytes=need - 1), -2, "workspace"),
                                ("null q", dict(q=None), -1, "null"), ("null ctx", dict(ctx=None), -1, "null"), ("null workspace", dict(ws=None), -1, "null"),
                                ("null host offsets", dict(off_host=False), -1, "batch"), ("ldq < D", dict(ld=60), -1, "leading"),
                                ("alpha with a huge aperture", dict(w=2 ** 30, alpha=fake(6), ws_bytes=1 << 40), -1, "alpha")]:
        rc = band(**kw)
        msg = lib.sumk_last_error().decode()
        assert rc == code and "attn_band" in msg and word in msg, (tag, rc, msg)

    wts = _lib.VasnetWeights(*[0x2000 * (k + 1) for k in range(10)])
    need = lib.sumk_vasnet_band_workspace_bytes(64, 1, _off([33]), 4)

    def fwd(lens=(33,), D_=64, w=4, precision=0, dropout_p=0.0, ws_bytes=need, x=fake(0)):
        lens = list(lens)
        o = _lib.VasnetOpts(0.125, 1e-6, 0, w, dropout_p, 0, precision, None, None, None, None, None)
        return lib.sumk_vasnet_forward_band(x, D_, len(lens), _off(lens), fake(1), C.byref(wts), C.byref(o), fake(2), fake(3), ws_bytes, None)

    for tag, kw, code, word in [("global attention", dict(w=-1), -1, "aperture"), ("bf16x6", dict(precision=2), -1, "fp32"), ("bf16x3", dict(precision=1), -1, "fp32"),
                                ("dropout", dict(dropout_p=0.5), -1, "dropout"), ("D=6", dict(D_=6), -1, "D=6"), ("T too long", dict(lens=[1048577], ws_bytes=1 << 40), -1, "steps"),
                                ("empty video", dict(lens=[0]), -1, "steps"), ("short workspace", dict(ws_bytes=need - 1), -2, "workspace"), ("null x", dict(x=None), -1, "null")]:
        rc = fwd(**kw)
        msg = lib.sumk_last_error().decode()
        assert rc == code and "vasnet_forward_band" in msg and word in msg, (tag, rc, msg)


def test_model_constructor_checks():
    from summarizer_amd._lib import SumkError
    from summarizer_amd.models.vasnet import VASNet
    for kw in (dict(), dict(attention_aperture=-1), dict(attention_aperture=2.5), dict(attention_aperture=8, fold_vo=True),
               dict(attention_aperture=8, precision="bf16x6"), dict(attention_aperture=8, precision="bf16x3")):
        with pytest.raises(SumkError, match="band"):
            VASNet(input_size=64, local_attention="band", **kw)
    with pytest.raises(SumkError, match="local_attention"):
        VASNet(input_size=64, attention_aperture=8, local_attention="banded")
    band, dense = VASNet(input_size=64, attention_aperture=8, local_attention="band"), VASNet(input_size=64, attention_aperture=8)
    assert band.local_attention == "band" and dense.local_attention == "dense"
    assert list(band.state_dict()) == list(dense.state_dict())                 # no new parameter
    assert VASNet(input_size=64, attention_aperture=0, local_attention="band").aperture == 0


def test_trainer_takes_local_attention():
    from summarizer_amd.models.vasnet import VASNetTrainer

    class _Hps:
        extra_params = {"local": "8", "local_attention": "band", "input_size": "64"}
        use_cuda = False
    t = VASNetTrainer.__new__(VASNetTrainer)
    t.hps = _Hps()
    m = t._init_model()
    assert m.local_attention == "band" and m.aperture == 8
    _Hps.extra_params = {"local": "8", "input_size": "64"}
    assert t._init_model().local_attention == "dense"


def test_chain_sums_equal_plain_products_at_float64():
    """The one-accumulator chain of the float32 yardstick is the same formula: at float64 it moves nothing above 1e-12."""
    lens = [65, 200, 2]
    parts = [_inputs(T, seed=9) for T in lens]
    Q, K, V = (np.concatenate([p[k] for p in parts]) for k in range(3))
    for w in (0, 31, 300):
        c0, a0 = attn_band_ref.band_attention(Q, K, V, lens, w, 0.25, False)
        c1, a1 = attn_band_ref.band_attention(Q, K, V, lens, w, 0.25, False, chain=True)
        assert np.array_equal(np.isnan(c0), np.isnan(c1)) and np.array_equal(np.isnan(a0), np.isnan(a1))
        assert (np.abs(np.nan_to_num(c0) - np.nan_to_num(c1)) <= 1e-12).all() and (np.abs(np.nan_to_num(a0) - np.nan_to_num(a1)) <= 1e-12).all()
