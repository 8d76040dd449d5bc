"""CPU: the pieces of banded KTS that need no GPU -- the O(n B) float64 specification tests/kts_banded_ref.py pinned against the (n x n)
reference tests/kts_ref.py, the size query sumk_kts_banded_workspace_bytes (pure host arithmetic) and the refusals of sumk_kts_banded, which
come before anything touches a device (made-up pointers, refused calls only)."""
import ctypes as C
import os

import numpy as np
import pytest

import kts_banded_ref
import kts_ref
from conftest import ROOT

LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")
SIZES = (1, 2, 33, 65, 130)
WINDOWS = ((1, 100000), (1, 1), (4, 40), (3, 64), (5, 7))


def _gram(n):
    rng = np.random.default_rng(300 + n)
    X = rng.standard_normal((n, 8))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X, X @ X.T


@pytest.mark.parametrize("lmin,lmax", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_banded_reference_equals_full_reference(n, lmin, lmax):
    """I, p, m_best, cps and scores of the band-only specification against kts_ref.dp / cpd_auto.  The two differ in summation order only
    (corner-started sums against global 2-D prefix sums): entries <= 1, n <= 130 -> 1e-10 relative to max(1, |.|) is orders above either's
    rounding and orders below any gap between distinct candidates of these random inputs, so p must be EQUAL."""
    X, K = _gram(n)
    B = kts_banded_ref.band_width(n, lmax)
    Kc = kts_banded_ref.band_from_gram(K, B)
    assert Kc.shape == (n, B)
    np.testing.assert_allclose(kts_banded_ref.band_from_features(X, B, block=32), Kc, rtol=0, atol=1e-14)
    J, Jb = kts_ref.scatter(K), kts_banded_ref.scatter_band(Kc)
    for c in range(B):
        np.testing.assert_allclose(Jb[:n - c, c], np.diagonal(J, c), rtol=0, atol=1e-10)
    for m in sorted({0, min(1, n - 1), min(5, n - 1), n - 1}):
        I, p = kts_ref.dp(K, m, lmin, lmax)
        Ib, pb = kts_banded_ref.dp_band(Jb, m, lmin, lmax)
        assert np.array_equal(I > 1e99, Ib > 1e99), (n, m)
        fin = I < 1e99
        assert (np.abs(I[fin] - Ib[fin]) <= 1e-10 * np.maximum(1.0, np.abs(I[fin]))).all(), (n, m)
        assert np.array_equal(p, pb), (n, m)
        for vmax in (1.0, 0.25):
            mb, cps, s, cost = kts_ref.cpd_auto(K, m, vmax, lmin, lmax, full=True)
            mb2, cps2, s2, cost2 = kts_banded_ref.cpd_auto(K, m, vmax, lmin, lmax, full=True)
            assert mb == mb2 and np.array_equal(cps, cps2) and np.array_equal(np.isinf(s), np.isinf(s2)), (n, m, vmax)
            f = np.isfinite(s)
            assert (np.abs(s[f] - s2[f]) <= 1e-10 * np.maximum(1.0, np.abs(s[f]))).all()
        rc, rs = kts_ref.cpd_nonlin(K, m, lmin, lmax)
        bc, bs = kts_banded_ref.cpd_nonlin_band(Kc, m, lmin, lmax)
        assert np.array_equal(rc, bc) and np.array_equal(np.isinf(rs), np.isinf(bs))


def test_banded_reference_from_features_matches_planted_boundaries():
    X, b = kts_ref.planted_features(130, 64, 7, 0.05, 3)
    cps, s = kts_banded_ref.cpd_auto_features(X, 129, lmax=60)
    K = X.astype(np.float64) @ X.astype(np.float64).T
    want, ws = kts_ref.cpd_auto(K, 129, lmax=60)
    assert cps.tolist() == want.tolist() == b.tolist()
    np.testing.assert_allclose(s, ws, rtol=0, atol=1e-10)


# ------------------------------------------------------------------------------------------------ the C entries, without a device
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(LIB)
    i32p = C.POINTER(C.c_int32)
    lib.sumk_kts_workspace_bytes.restype = C.c_size_t
    lib.sumk_kts_workspace_bytes.argtypes = [C.c_int32, C.c_int32, i32p, C.c_int32]
    lib.sumk_kts_banded_workspace_bytes.restype = C.c_size_t
    lib.sumk_kts_banded_workspace_bytes.argtypes = [C.c_int32, C.c_int32, i32p, C.c_int32, C.c_int32]
    lib.sumk_kts_banded.restype = C.c_int
    lib.sumk_kts_banded.argtypes = [C.c_void_p, C.c_int32, C.c_int32, i32p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.sumk_last_error.restype = C.c_char_p
    return lib


def _off(lens):
    return (C.c_int32 * (len(lens) + 1))(*np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist())


def test_workspace_query_needs_no_gpu(lib):
    q = lambda D, lens, m, lmax: lib.sumk_kts_banded_workspace_bytes(D, len(lens), _off(lens), m, lmax)
    dense = lambda D, lens, m: lib.sumk_kts_workspace_bytes(D, len(lens), _off(lens), m)
    # less than the dense path whenever lmax < n (same batch, same max_ncp), at every length both take
    for n in (130, 300, 1025, 4200, 16384):
        for lmax in (1, 7, 40, n // 2, n - 1):
            assert 0 < q(64, [n], 12, lmax) < dense(64, [n], 12), (n, lmax)
    assert 0 < q(64, [33, 130, 700], 40, 20) < dense(64, [33, 130, 700], 40)
    # it holds the float64 band and, in one shared region, the fp32 strips or the int32 back-pointers with two I rows, whichever is larger
    for n, B, m in ((5000, 300, 40), (5000, 30, 999)):
        low = n * B * 8 + max(n * (B + 63) * 4, m * (n + 1) * 4 + 2 * (n + 1) * 8)
        assert low <= q(64, [n], m, B) <= low + n * 8 + 2 * n * 4 + 64 * 1024, (n, B, m)
    # grows as n B: doubling n or B doubles the band term; past lmax >= n nothing grows any more
    base = q(64, [8192], 0, 256)
    assert abs(q(64, [16384], 0, 256) / base - 2.0) < 0.02 and abs(q(64, [8192], 0, 512) / base - 2.0) < 0.2
    assert q(64, [8192], 0, 512) > base and q(64, [8192], 40, 256) > base
    assert q(64, [300], 12, 300) == q(64, [300], 12, 100000) == q(64, [300], 12, 2 ** 31 - 1)
    assert q(1024, [300], 12, 40) == q(64, [300], 12, 40)                          # D decides nothing but eligibility
    # a video the dense path refuses: 1 048 576 steps in a band of 64 is ~1 GB, not n^2
    big = q(64, [1048576], 100, 64)
    assert 1048576 * 64 * 8 < big < 2 * 1048576 * 64 * 8 + 1048576 * 101 * 4 and dense(64, [1048576], 100) == 0
    assert q(64, [1, 2, 65], 64, 3) > 0 and q(64, [1], 0, 1) > 0
    for bad in ((64, [1048577], 0, 10), (6, [130], 12, 10), (0, [130], 12, 10), (64, [130], -1, 10), (64, [130], 130, 10), (64, [130, 0], 1, 10),
                (64, [130], 12, 0), (64, [130], 12, -3)):
        assert q(*bad) == 0, bad
    assert lib.sumk_kts_banded_workspace_bytes(64, 0, _off([]), 0, 10) == 0
    assert lib.sumk_kts_banded_workspace_bytes(64, 1, None, 0, 10) == 0


def test_refusals_launch_nothing(lib):
    """Every refused call returns SUMK_ERR_ARG (-1) with a message before it touches its pointers: these are made up."""
    fake = lambda k: C.c_void_p(0x1000 * (k + 1))
    need = lib.sumk_kts_banded_workspace_bytes(64, 1, _off([33]), 32, 40)
    assert need > 0

    def call(lens=(33,), D=64, max_ncp=32, lmin=1, lmax=40, ws_bytes=need, x=fake(0), off_dev=fake(1), n_cps=fake(2), cps=fake(3), ws=fake(5),
             off_host=True):
        lens = list(lens)
        return lib.sumk_kts_banded(x, D, len(lens), _off(lens) if off_host else None, off_dev, max_ncp, lmin, lmax, 1.0, n_cps, cps, fake(4), ws,
                                   ws_bytes, None)

    bad = [("n=1048577", dict(lens=[1048577], max_ncp=3, ws_bytes=1 << 40), "steps"), ("lmin=0", dict(lmin=0), "lmin"),
           ("lmax<lmin", dict(lmin=5, lmax=4), "lmin"), ("D=6", dict(D=6), "D=6"), ("max_ncp=n", dict(max_ncp=33), "max_ncp"),
           ("max_ncp<0", dict(max_ncp=-1), "max_ncp"), ("short workspace", dict(ws_bytes=need - 1), "workspace"),
           ("null x", dict(x=None), "null"), ("null offsets", dict(off_dev=None), "null"), ("null n_cps", dict(n_cps=None), "null"),
           ("null cps", dict(cps=None), "null"), ("null workspace", dict(ws=None), "null"), ("null host offsets", dict(off_host=False), "batch")]
    for tag, kw, word in bad:
        rc = call(**kw)
        msg = lib.sumk_last_error().decode()
        assert rc == -1 and "kts_banded" in msg and word in msg, (tag, rc, msg)
