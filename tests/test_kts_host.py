"""CPU: the pieces of the KTS feature that need no GPU -- the float64 reference tests/kts_ref.py pinned against brute-force enumeration of
every placement, the step -> frame conversion utils.kts.cps_to_segments, and the size query sumk_kts_workspace_bytes (pure host arithmetic)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import kts_ref
from conftest import ROOT

LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")


def _brute(K, m, lmin, lmax):
    """(best objective, its change points) over every placement of m change points the recurrence admits: the i-th boundary (1-based, the
    end n counting as boundary m + 1) lies at or after i * lmin, the first segment is shorter than lmax (exclusive: the original's quirk) and
    every later one at most lmax long."""
    n = K.shape[0]
    J = kts_ref.scatter(K)
    best = (np.inf, None)
    for cps in itertools.combinations(range(1, n), m):
        b = (0,) + cps + (n,)
        lens = np.diff(b)
        if any(b[i] < i * lmin for i in range(1, m + 2)) or lens[1:].max(initial=0) > lmax or lens[0] >= lmax:
            continue
        v = sum(J[b[q], b[q + 1] - 1] for q in range(m + 1))
        if v < best[0]:
            best = (v, cps)
    return best


@pytest.mark.parametrize("lmin,lmax", [(1, 100000), (2, 4)])
def test_reference_equals_brute_force(lmin, lmax):
    rng = np.random.default_rng(5)
    for n in range(1, 10):
        X = rng.standard_normal((n, 6))
        K = X @ X.T
        for m in range(0, min(3, n - 1) + 1):
            want, want_cps = _brute(K, m, lmin, lmax)
            cps, scores = kts_ref.cpd_nonlin(K, m, lmin, lmax)
            assert scores.shape == (m + 1,) and cps.shape == (m,)
            if not np.isfinite(want):
                assert np.isinf(scores[m]), (n, m)
                continue
            assert abs(scores[m] - want) <= 1e-12 * max(1.0, abs(want)), (n, m, scores[m], want)
            assert abs(kts_ref.objective(K, cps) - want) <= 1e-12 * max(1.0, abs(want)), (n, m, cps, want_cps)


def test_reference_auto_picks_smallest_cost():
    X, b = kts_ref.planted_features(65, 64, 5, 0.05, 3)
    K = X.astype(np.float64) @ X.astype(np.float64).T
    mb, cps, s, cost = kts_ref.cpd_auto(K, 64, full=True)
    assert mb == 4 and cps.tolist() == b.tolist()
    assert mb == int(np.argmin(cost)) and np.all(np.diff(s[np.isfinite(s)]) <= 1e-12)      # more change points never raise the scatter
    cps2, s2 = kts_ref.cpd_auto(K, 64)
    assert cps2.tolist() == cps.tolist() and np.array_equal(s2, s[:mb + 1])


def test_cps_to_segments():
    from summarizer_amd.utils.kts import cps_to_segments
    rng = np.random.default_rng(9)
    for n, m in ((1, 0), (7, 0), (7, 3), (40, 9), (40, 39)):
        picks = np.sort(rng.choice(np.arange(0, 15 * n), n, replace=False)).astype(np.int32)       # irregular
        picks[0] = 0 if m == n - 1 else picks[0]
        n_frames = int(picks[-1]) + int(rng.integers(1, 20))
        cps = np.sort(rng.choice(np.arange(1, n), m, replace=False)) if m else np.array([], dtype=np.int64)
        seg, nfps = cps_to_segments(cps, picks, n_frames)
        assert seg.dtype == np.int32 and nfps.dtype == np.int32 and seg.shape == (m + 1, 2) and nfps.shape == (m + 1,)
        assert seg[0, 0] == 0 and seg[-1, 1] == n_frames - 1
        assert np.array_equal(seg[1:, 0], seg[:-1, 1] + 1)                                          # no gap, no overlap
        assert np.array_equal(seg[1:, 0], picks[cps])                                               # boundaries = picks[c]
        assert np.array_equal(nfps, seg[:, 1] - seg[:, 0] + 1) and nfps.sum() == n_frames and (nfps > 0).all()
        cover = np.zeros(n_frames, dtype=np.int64)
        for lo, hi in seg:
            cover[lo:hi + 1] += 1
        assert (cover == 1).all()
    seg, nfps = cps_to_segments([], np.arange(5), 5)
    assert seg.tolist() == [[0, 4]] and nfps.tolist() == [5]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(LIB)
    lib.sumk_kts_workspace_bytes.restype = C.c_size_t
    lib.sumk_kts_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    return lib


def _off(lens):
    return (C.c_int32 * (len(lens) + 1))(*np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist())


def test_workspace_query_needs_no_gpu(lib):
    q = lambda D, lens, m: lib.sumk_kts_workspace_bytes(D, len(lens), _off(lens), m)
    base = q(64, [130], 12)
    assert base >= 130 * 130 * 8 + 12 * 131                     # J in float64 and the back-pointers at least
    assert q(64, [130], 40) > base and q(64, [130], 129) > q(64, [130], 40)          # grows with max_ncp
    assert q(64, [260], 12) > base and q(64, [130, 130], 12) > base                  # and with n
    assert q(1024, [130], 12) == base                                               # D decides nothing but eligibility
    assert q(64, [16384], 0) > 16384 * 16384 * 8
    assert q(64, [1, 2, 65], 64) > 0 and q(64, [1], 0) > 0
    for bad in ((64, [16385], 0), (6, [130], 12), (0, [130], 12), (64, [130], -1), (64, [130], 130), (64, [130, 0], 1)):
        assert q(*bad) == 0, bad
    assert lib.sumk_kts_workspace_bytes(64, 0, _off([]), 0) == 0
    assert lib.sumk_kts_workspace_bytes(64, 1, None, 0) == 0
