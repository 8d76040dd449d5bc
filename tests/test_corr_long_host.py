"""CPU: the host side of the long-video rank correlation (csrc/evalcorr_long.hip) -- the four symbols, the workspace arithmetic of
sumk_eval_device_spearman_long / sumk_eval_device_kendall_long against its Python mirror, `corr_long_refusal` in words, the `tail`
argument of evaluate_batch_device, and the exact Spearman oracle of tests/corr_long_common.py against the host tail (the GPU tests of
tests/test_gpu_corr_long.py measure the device's distance from that oracle)."""
import ctypes as C
import time

import numpy as np
import pytest

import corr_long_common as K

NAMES = ("sumk_eval_device_spearman_long_workspace_bytes", "sumk_eval_device_spearman_long", "sumk_eval_device_kendall_long_workspace_bytes",
         "sumk_eval_device_kendall_long")


def _descr(geometries):
    """Host descriptors of videos of (n_picks, n_frames, n_users): the size queries read nothing else but the picks pointer's presence."""
    from summarizer_amd import _lib
    d = (_lib.EvalDevVideo * max(len(geometries), 1))()
    for e, (p, f, u) in zip(d, geometries):
        e.picks, e.n_picks, e.n_frames, e.n_users = 0x1000, p, f, u
    return d


def test_symbols_are_exported_and_bound():
    from summarizer_amd import _lib, kernels
    from summarizer_amd.utils import eval_native
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib._SIGS and hasattr(lib, name), name
    for name in ("eval_spearman_long_workspace_bytes", "eval_spearman_long", "eval_kendall_long_workspace_bytes", "eval_kendall_long"):
        assert callable(getattr(kernels, name)), name
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "sumk.h")).read()
    assert f"#define SUMK_CORR_LONG_TILE {eval_native.CORR_LONG_TILE}" in header and eval_native.CORR_LONG_TILE == K.TILE


def test_workspace_bytes_equal_the_python_mirror_and_refuse_bad_geometries():
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    lib = _lib.load()
    T = K.TILE
    table = [[(1, 1, 0)], [(1, 16, 3)], [(4096, 61440, 20)], [(4097, 61455, 32)], [(T - 1, 15 * T, 1), (T, 15 * T, 2), (T + 1, 15 * T + 20, 3)],
             [(5 * T + 3, 153645, 32), (1, 16, 1)], [(65536, 983040, 20)], [(1 << 20, 1 << 24, 32)], [(7200, 108000, 20)] * 63,
             [(1023, 100, -1)], [(1024, 5000, 0)], [(300, 4097, 5), (2, 40, 32), (1, 1 << 24, 1)]]
    for geoms in table:
        d = _descr(geoms)
        for metric, fn in (("spearmanr", lib.sumk_eval_device_spearman_long_workspace_bytes), ("kendalltau", lib.sumk_eval_device_kendall_long_workspace_bytes)):
            got = fn(C.cast(d, C.c_void_p), len(geoms))
            assert got > 0 and got == eval_native.corr_long_workspace_bytes(geoms, metric), (geoms[:3], metric, got)
    # Kendall: 16 bytes per (annotator, frame) dominate; Spearman stays near 36 bytes per group
    one = _descr([(65536, 983040, 20)])
    kb = lib.sumk_eval_device_kendall_long_workspace_bytes(C.cast(one, C.c_void_p), 1)
    sb = lib.sumk_eval_device_spearman_long_workspace_bytes(C.cast(one, C.c_void_p), 1)
    assert 16 * 20 * 983040 < kb < 16 * 20 * 983040 + (4 << 20) and sb < (4 << 20)
    for bad in ([(0, 10, 1)], [((1 << 20) + 1, 10, 1)], [(10, 0, 1)], [(10, (1 << 24) + 1, 1)], [(10, 10, 33)], [(5, 50, 2), (5, 50, 33)]):
        d = _descr(bad)
        for metric, fn in (("spearmanr", lib.sumk_eval_device_spearman_long_workspace_bytes), ("kendalltau", lib.sumk_eval_device_kendall_long_workspace_bytes)):
            assert fn(C.cast(d, C.c_void_p), len(bad)) == 0 and eval_native.corr_long_workspace_bytes(bad, metric) == 0, (bad, metric)
    ok = _descr([(5, 50, 2)])
    for fn in (lib.sumk_eval_device_spearman_long_workspace_bytes, lib.sumk_eval_device_kendall_long_workspace_bytes):
        assert fn(C.cast(ok, C.c_void_p), 0) == 0 and fn(C.cast(ok, C.c_void_p), -1) == 0 and fn(None, 1) == 0 and fn(C.cast(ok, C.c_void_p), 65536) == 0


def test_corr_long_refusal_names_each_limit():
    from summarizer_amd.utils.eval_native import corr_long_refusal
    assert corr_long_refusal(1, 1, 0) is None and corr_long_refusal(1 << 20, 1 << 24, 32) is None and corr_long_refusal(65536, 983040, 20) is None
    assert "0 picks (1 .. 1048576)" in corr_long_refusal(0, 100, 1)
    assert "1048577 picks (1 .. 1048576)" in corr_long_refusal((1 << 20) + 1, 100, 1)
    assert "0 frames (1 .. 16777216)" in corr_long_refusal(10, 0, 1)
    assert "16777217 frames (1 .. 16777216)" in corr_long_refusal(10, (1 << 24) + 1, 1)
    assert "33 annotators (at most 32)" in corr_long_refusal(10, 100, 33)


def test_device_ready_long_takes_what_the_block_tail_declines():
    from summarizer_amd.utils import eval_native
    v = K.prepare(K.make_video(4200, 1))
    assert eval_native.device_ready_long(v) and not eval_native.device_ready(v)
    long_frames = K.prepare(K.video_of_frames(16385, 2))
    assert eval_native.device_ready_long(long_frames) and eval_native.device_ready(long_frames) and not eval_native.kendall_device_ready(long_frames)
    raw = K.make_video(60, 3)
    shuffled = dict(raw, picks=raw["picks"][::-1].copy())
    assert not eval_native.device_ready_long(K.prepare(shuffled))
    assert not eval_native.device_ready_long(eval_native.prepare_video(raw["n_frames"], raw["picks"]))


def test_unknown_tail_is_rejected_before_the_gpu_is_touched():
    from summarizer_amd.utils import eval_native

    class NotATensor:
        def __getattr__(self, name):
            raise AssertionError(f"the scores were looked at ({name}) before the tail was checked")
    with pytest.raises(KeyError, match="Unknown tail tall"):
        eval_native.evaluate_batch_device([], NotATensor(), [], tail="tall")
    assert eval_native.TAILS == ("block", "long")


def test_exact_spearman_oracle_agrees_with_the_host_tail():
    from summarizer_amd.utils import eval_native
    raws = [K.make_video(p, 40 + i, n_users=u, tail=t) for i, (p, u, t) in enumerate([(1, 3, 9), (2, 2, 0), (40, 5, 9), (333, 4, 0), (1200, 7, 4)])]
    vids = [K.prepare(r) for r in raws]
    host = eval_native.evaluate_batch(vids, [r["scores"] for r in raws], n_threads=2)[0]
    ref = np.array([K.exact_spearman(r["scores"], r["n_frames"], r["picks"], v["user_ranks"]) for r, v in zip(raws, vids)])
    assert np.array_equal(np.isnan(host), np.isnan(ref)) and np.isfinite(ref).sum() >= 3      # (one pick, one interval: a constant side is NaN on both)
    ok = np.isfinite(ref)
    assert np.abs(host[ok] - ref[ok]).max() <= 1e-12
    # an independent check of the oracle itself: scipy on the upsampled scores
    from scipy import stats
    r = raws[3]
    fs = K.frame_scores(r["scores"], r["n_frames"], r["picks"])
    want = np.mean([stats.spearmanr(fs, r["user_scores"][u])[0] for u in range(r["user_scores"].shape[0])])
    assert abs(ref[3] - want) <= 1e-12
    # the size the GPU test uses: seconds on the CPU
    big = K.video_of_frames(300000, 77, n_users=4)
    t0 = time.perf_counter()
    x = K.exact_spearman(big["scores"], big["n_frames"], big["picks"], K.prepare(big)["user_ranks"])
    assert np.isfinite(x) and time.perf_counter() - t0 < 30.0
