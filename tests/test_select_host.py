"""CPU: the host side of key-shot selection on the device (csrc/evalselect.hip) -- the numpy specification of the padded segment layout
and the premise it rests on (empty segments never change a summary), the workspace arithmetic, the `select_device_ready` predicate, and
the new symbols in the header, the ctypes table and the cross-compiled library.  The kernels themselves: tests/test_gpu_select.py."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from summarizer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_padded_segments_are_the_live_ones_followed_by_empty_ones():
    from summarizer_amd.utils import kts
    rng = np.random.default_rng(3)
    for T, n_cps, n_segs in ((40, 0, 1), (40, 0, 7), (130, 5, 6), (130, 5, 64), (300, 17, 1024)):
        picks = (3 * np.arange(T) + rng.integers(0, 3)).astype(np.int32)
        n_frames = int(picks[-1]) + 4
        cps = np.sort(rng.choice(np.arange(1, T), size=n_cps, replace=False))
        cp, nfps = kts.cps_to_segments(cps, picks, n_frames)
        cpp, nfpsp = kts.cps_to_segments_padded(cps, picks, n_frames, n_segs)
        assert cpp.shape == (n_segs, 2) and nfpsp.shape == (n_segs,) and cpp.dtype == np.int32 and nfpsp.dtype == np.int32
        np.testing.assert_array_equal(cpp[:n_cps + 1], cp)
        np.testing.assert_array_equal(nfpsp[:n_cps + 1], nfps)
        assert (cpp[n_cps + 1:] == [n_frames, n_frames - 1]).all() and (nfpsp[n_cps + 1:] == 0).all()
        assert int(nfpsp.sum()) == n_frames
    with pytest.raises(ValueError):
        kts.cps_to_segments_padded([5, 9], np.arange(20), 20, 2)


def _premise_cases():
    """(scores, picks, n_frames, live segments, padded segments) on random videos; tied=True draws the scores from a few values so that
    most optima are tied, with runs of exact zeros (the pads' own mean)."""
    from summarizer_amd.utils import kts
    rng = np.random.default_rng(17)
    for trial in range(40):
        T = int(rng.integers(2, 200))
        picks = (2 * np.arange(T)).astype(np.int32)
        n_frames = 2 * T + int(rng.integers(0, 2))
        n_cps = int(rng.integers(0, min(T - 1, 30) + 1))
        cps = np.sort(rng.choice(np.arange(1, T), size=n_cps, replace=False))
        tied = rng.choice(np.array([0.0, 0.25, 0.5, -0.5], np.float32), size=T)
        if trial % 3 == 0:
            tied[:] = 0.0 if trial % 2 else 0.25
        distinct = rng.standard_normal(T).astype(np.float32)
        live = kts.cps_to_segments(cps, picks, n_frames)
        padded = kts.cps_to_segments_padded(cps, picks, n_frames, n_cps + 1 + int(rng.integers(1, 40)))
        yield tied, distinct, picks, n_frames, live, padded


@pytest.mark.parametrize("method", ["knapsack", "rank"])
def test_empty_segments_do_not_change_a_summary(lib, method):
    """The premise of the padded layout.  generate_summary (the numpy specification + the native knapsack) on the live segments and on
    the same segments padded with empty ones: equal -- for the knapsack with heavily tied scores, for rank with distinct ones (numpy's
    argsort is not stable, so among EQUAL segment scores the numpy rank walk has no order to keep once the array grows; the order the
    project pins, std::stable_sort's, is the native host tail's, next).  Then the native host tail itself, the reference of the device
    path, with tied scores and both methods."""
    import warnings
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native as N
    for tied, distinct, picks, n_frames, (cp, nfps), (cpp, nfpsp) in _premise_cases():
        for proportion in (0.15, 0.5, 1.0):
            scores = tied if method == "knapsack" else distinct
            with np.errstate(invalid="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")                 # (numpy's mean of an empty segment is NaN, with a warning)
                a = E.generate_summary(scores, cp, n_frames, nfps.tolist(), picks, proportion, method)
                b = E.generate_summary(scores, cpp, n_frames, nfpsp.tolist(), picks, proportion, method)
            np.testing.assert_array_equal(a, b)
            vids = [N.prepare_video(n_frames, picks, cp, nfps), N.prepare_video(n_frames, picks, cpp, nfpsp)]
            got = N.evaluate_batch(vids, [tied, tied], proportion, method, want_summaries=True, n_threads=1)[3]
            np.testing.assert_array_equal(got[0], got[1])
            if method == "knapsack":
                np.testing.assert_array_equal(got[0], E.generate_summary(tied, cp, n_frames, nfps.tolist(), picks, proportion, method))


def test_workspace_bytes_arithmetic(lib):
    f = lib.sumk_eval_device_select_workspace_bytes
    up = lambda x: (x + 255) // 256 * 256
    # per video: one bit per (segment, capacity 0 .. max) in 64-bit words, rounded to 256 bytes; above the LDS capacity, two int32 rows more
    assert f(1, 1, 0) == 256
    assert f(3, 10, 63) == 3 * up(10 * 8) and f(3, 10, 64) == 3 * up(10 * 16)
    assert f(50, 64, 2000) == 50 * up(64 * 32 * 8)
    assert f(2, 1024, 4095) == 2 * 1024 * 64 * 8
    assert f(2, 1024, 4096) == 2 * (up(1024 * 65 * 8) + up(2 * 4097 * 4))
    assert f(1, 1024, 8191) == 1024 * 128 * 8 + 2 * 8192 * 4
    for bad in ((0, 1, 1), (-1, 1, 1), (1, 0, 1), (1, 1025, 1), (1, 1, -1), (1, 1, 8192)):
        assert f(*bad) == 0, bad


def test_select_device_ready_mirrors_the_limits():
    from summarizer_amd.utils import eval_native as N

    def video(n_frames, n_segs, n_users, **over):
        nfps = np.zeros(n_segs, np.int32); nfps[0] = n_frames
        cps = np.zeros((n_segs, 2), np.int32); cps[:, 1] = n_frames - 1
        v = N.prepare_video(n_frames, np.arange(0, n_frames, 15), cps, nfps, np.zeros((n_users, n_frames), np.float32) if n_users else None)
        v.update(over)
        return v
    assert (N.SELECT_MAX_SEGS, N.SELECT_MAX_CAPACITY, N.SELECT_MAX_USERS, N.SELECT_LDS_CAPACITY) == (1024, 8191, 32, 4095)
    assert N.select_device_ready(video(300, 5, 3)) and N.select_device_ready(video(300, 5, 0)) and N.select_device_ready(video(300, 1024, 32))
    assert not N.select_device_ready(video(300, 1025, 3))                   # one segment over
    assert not N.select_device_ready(video(300, 5, 33))                     # one annotator over
    assert N.select_capacity(54613, 0.15) == 8191 and N.select_device_ready(video(54613, 2, 1), 0.15)
    assert N.select_capacity(54614, 0.15) == 8192 and not N.select_device_ready(video(54614, 2, 1), 0.15)
    assert N.select_device_ready(video(8191, 2, 1), 1.0) and not N.select_device_ready(video(8192, 2, 1), 1.0)
    assert not N.select_device_ready(video(300, 5, 3), -0.1)                # a negative budget
    assert not N.select_device_ready(N.prepare_video(300, np.arange(20)))   # no change points
    assert not N.select_device_ready(video(300, 5, 3, nfps=np.array([300, 0, -1, 1, 0], np.int32)))
    assert not N.select_device_ready(video(300, 5, 3, user_summary=np.zeros((3, 299), np.float32)))
    # the budget is eval_one's: floor of the DOUBLE product
    for n_frames, p in ((100, 0.15), (20, 0.15), (4520, 0.15), (7, 1 / 3)):
        assert N.select_capacity(n_frames, p) == int(np.floor(np.float64(n_frames) * np.float64(p)))
    assert N.select_refusal(1025, 300, 0, 0.15) is not None and "segments" in N.select_refusal(1025, 300, 0, 0.15)


def test_new_symbols_are_declared_bound_and_exported(lib):
    from summarizer_amd import _lib
    header = open(os.path.join(ROOT, "include", "sumk.h")).read()
    exported = C.CDLL(_lib.LIB_PATH)
    for name in ("sumk_eval_device_select", "sumk_eval_device_select_workspace_bytes", "sumk_kts_segments"):
        assert name + "(" in header and name in _lib._SIGS and hasattr(exported, name), name
    for macro, value in (("SUMK_SELECT_MAX_SEGS", 1024), ("SUMK_SELECT_MAX_CAPACITY", 8191), ("SUMK_SELECT_LDS_CAPACITY", 4095),
                         ("SUMK_SELECT_MAX_USERS", 32)):
        assert f"#define {macro} {value}" in header
    assert C.sizeof(_lib.EvalDevSelect) == 64          # two pointers, four int32, two int64, a pointer, two int32
    with pytest.raises(KeyError):
        from summarizer_amd.utils import eval_native
        eval_native.evaluate_batch_device([], None, [], select="somewhere")
