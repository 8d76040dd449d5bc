"""GPU: key-shot selection, summary expansion and F-scores on the device (csrc/evalselect.hip: sumk_eval_device_select, sumk_kts_segments),
`evaluate_batch_device(select="device")`, `Summarizer(device=True)` and the `hps.selection_device` opt-in of the trainers.

The reference throughout is the host tail -- `sumk_eval_videos` with the segment means given, `eval_native.evaluate_batch`,
`sumk_knapsack_dp` -- and every comparison is `assert_array_equal`: the device path has to reproduce the host's integers, its tie
rules and its float32 / float64 F-score arithmetic bit for bit, so no tolerance appears anywhere in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

import recipes as R

pytestmark = pytest.mark.gpu

LDS_CAP = 4095           # SUMK_SELECT_LDS_CAPACITY: the largest budget whose profit rows stay in LDS


def _dev():
    return torch.device("cuda:0")


def _poisoned(numel, dtype, dev):
    t = torch.empty(max(int(numel), 1), dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(255)
    return t


def _select_call(vids, method, gap=3, ws_short=0, override=None, dev_override=None):
    """sumk_eval_device_select on buffers of the test's own, all of them -- the workspace too -- filled with 0xFF bytes first.
    vids: dicts with means (S,) float32, nfps (S,) int32, n_frames, capacity and mask (U, n_frames) uint8 or None; the videos' ranges in
    the summary buffer are `gap` entries apart.  override: {video: {field: value}} on the HOST AND DEVICE copy of the descriptors;
    dev_override: the same on the device copy alone (what the entry point cannot see)."""
    from summarizer_amd import _lib
    lib, dev, n = _lib.load(), _dev(), len(vids)
    means = torch.from_numpy(np.concatenate([v["means"] for v in vids]).astype(np.float32)).to(dev)
    nfps = torch.from_numpy(np.concatenate([v["nfps"] for v in vids]).astype(np.int32)).to(dev)
    masks = [torch.from_numpy(np.ascontiguousarray(v["mask"])).to(dev) if v.get("mask") is not None else None for v in vids]
    descr = (_lib.EvalDevSelect * n)()
    seg_at, at, ranges = 0, gap, []
    for i, v in enumerate(vids):
        e, S = descr[i], len(v["means"])
        e.seg_means, e.nfps = means.data_ptr() + 4 * seg_at, nfps.data_ptr() + 4 * seg_at
        e.n_segs, e.n_frames, e.capacity, e.summary_len = S, int(v["n_frames"]), int(v["capacity"]), int(np.sum(v["nfps"], dtype=np.int64))
        e.summary0, e.sel0, e.method = at, seg_at, method
        if masks[i] is not None:
            e.user_mask, e.n_users = masks[i].data_ptr(), masks[i].shape[0]
        for k, val in (override or {}).get(i, {}).items():
            setattr(e, k, val)
        ranges.append((at, at + e.summary_len))
        at += e.summary_len + gap; seg_at += S
    on_dev = (_lib.EvalDevSelect * n).from_buffer_copy(bytes(descr))
    for i, fields in (dev_override or {}).items():
        for k, val in fields.items():
            setattr(on_dev[i], k, val)
    descr_dev = torch.frombuffer(bytearray(bytes(on_dev)), dtype=torch.uint8).to(dev)
    max_segs, max_cap = max(len(v["means"]) for v in vids), max(int(v["capacity"]) for v in vids)
    ws_bytes = lib.sumk_eval_device_select_workspace_bytes(n, min(max_segs, 1024), max_cap)
    assert ws_bytes > 0
    summary, selected = _poisoned(at, torch.float32, dev), _poisoned(seg_at, torch.uint8, dev)
    f_avg, f_max, status = _poisoned(n, torch.float64, dev), _poisoned(n, torch.float64, dev), _poisoned(n, torch.int32, dev)
    ws = _poisoned(ws_bytes, torch.uint8, dev)
    rc = lib.sumk_eval_device_select(descr_dev.data_ptr(), C.cast(descr, C.c_void_p), n, summary.data_ptr(), at, selected.data_ptr(), seg_at,
                                     f_avg.data_ptr(), f_max.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes - ws_short,
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    raw = summary.cpu().numpy()
    sel = selected.cpu().numpy()
    seg_off = np.concatenate([[0], np.cumsum([len(v["means"]) for v in vids])])
    outside = np.ones(raw.shape[0], bool)
    for lo, hi in ranges:
        outside[lo:hi] = False
    return dict(rc=rc, summaries=[raw[lo:hi] for lo, hi in ranges], selected=[sel[seg_off[i]:seg_off[i + 1]] for i in range(n)],
                f_avg=f_avg.cpu().numpy(), f_max=f_max.cpu().numpy(), status=status.cpu().numpy(), raw=raw, outside=outside, raw_selected=sel,
                error=lib.sumk_last_error().decode(errors="replace"))


def _host_tail(vids, proportion, method):
    """The reference: sumk_eval_videos with seg_means given (csrc/evaltail.hip eval_one) -> (summaries, f_avg, f_max)."""
    from summarizer_amd import _lib
    lib, n = _lib.load(), len(vids)
    arr = (_lib.EvalVideo * n)()
    keep, outs = [], []
    for i, v in enumerate(vids):
        e = arr[i]
        m, w = np.ascontiguousarray(v["means"], np.float32), np.ascontiguousarray(v["nfps"], np.int32)
        cps = np.zeros((len(m), 2), np.int32)
        out = np.full(int(w.sum(dtype=np.int64)), -7, np.float32)
        keep += [m, w, cps]; outs.append(out)
        e.n_frames, e.n_steps, e.cps, e.nfps, e.n_segs, e.seg_means = int(v["n_frames"]), 1, cps.ctypes.data, w.ctypes.data, len(m), m.ctypes.data
        e.machine_summary = out.ctypes.data
        if v.get("mask") is not None:
            us = np.ascontiguousarray(v["mask"], np.float32); keep.append(us)
            e.user_summary, e.n_users = us.ctypes.data, us.shape[0]
    _lib.check(lib.sumk_eval_videos(C.cast(arr, C.c_void_p), n, float(proportion), method, 0), "sumk_eval_videos")
    return outs, np.array([arr[i].f_avg for i in range(n)]), np.array([arr[i].f_max for i in range(n)])


def _expected_selected(v, method):
    """The selected set from the definitions: sumk_knapsack_dp on the integers eval_one builds / the stable rank walk."""
    from summarizer_amd import _lib
    lib = _lib.load()
    x = np.asarray(v["means"], np.float32).astype(np.float64)
    w = np.asarray(v["nfps"], np.int64)
    sel = np.zeros(len(x), np.uint8)
    if method == 0:
        vals = np.ascontiguousarray(np.trunc(x * 1000.0).astype(np.int64)); w = np.ascontiguousarray(w)
        _lib.check(lib.sumk_knapsack_dp(vals.ctypes.data_as(C.POINTER(C.c_int64)), w.ctypes.data_as(C.POINTER(C.c_int64)), len(x), int(v["capacity"]),
                                        sel.ctypes.data_as(C.POINTER(C.c_uint8))), "sumk_knapsack_dp")
    else:
        used = 0
        for i in np.argsort(x, kind="stable")[::-1]:
            if used + w[i] < v["capacity"]:
                sel[i] = 1; used += int(w[i])
    return sel


def _check(got, vids, proportion, method, what=""):
    assert got["rc"] == 0, got["error"]
    assert (got["status"] == 0).all(), (what, got["status"])
    summaries, f_avg, f_max = _host_tail(vids, proportion, method)
    for i, v in enumerate(vids):
        np.testing.assert_array_equal(got["selected"][i], _expected_selected(v, method), err_msg=f"{what} video {i} ({v.get('name')})")
        np.testing.assert_array_equal(got["summaries"][i], summaries[i], err_msg=f"{what} video {i} ({v.get('name')})")
    np.testing.assert_array_equal(got["f_avg"], f_avg, err_msg=what)
    np.testing.assert_array_equal(got["f_max"], f_max, err_msg=what)
    assert (got["raw"][got["outside"]].view(np.uint32) == 0xFFFFFFFF).all(), what          # nothing written outside the videos' ranges


# ------------------------------------------------------------------------------------------------ 1. integer problems through the C entry
SEGS = (1, 2, 63, 64, 65, 257, 1024)
CAPS = (0, 1, 63, 64, 1023, 1024, LDS_CAP, LDS_CAP + 1, 8191)      # capacity + 1 in {1, 2, 64, 65, 1024, 1025}, the LDS threshold and above, the limit


def _problems(cap, seed):
    """One budget, every segment count, the contents that decide ties and quirks.  n_frames = the budget (proportion 1; budget 0: one frame
    at proportion 0.5), so summaries are shorter than, equal to and longer than the video: both F-score branches."""
    rng = np.random.default_rng(seed)
    n_frames = max(cap, 1)
    out = []
    for S in SEGS:
        wmax = max(1, cap // 3)
        tied = rng.choice(np.array([0.0, 0.25, 0.5], np.float32), size=S)
        # (weights in the upper half of [1, budget / 3]: a handful of key shots per video, so the host reference, which re-solves its
        #  DP once per selected item, stays quick at 1024 segments x 8192 capacities; small budgets leave many EQUAL weights: tied optima)
        w = rng.integers(max(1, wmax // 2), wmax + 1, size=S).astype(np.int32)
        base = dict(n_frames=n_frames, capacity=cap)
        out.append(dict(base, name="tied", means=tied, nfps=w))
        neg = rng.choice(np.array([-0.5, -0.25, 0.0, 0.25, 0.5], np.float32), size=S)
        w2 = w.copy(); w2[rng.integers(0, S, size=min(3, S))] = 0                                   # some nfps = 0
        out.append(dict(base, name="negative+zero_weights", means=neg, nfps=w2))
        w3 = w.copy(); w3[0] = cap + 1                                                              # item 0 heavier than the capacity
        m3 = tied.copy(); m3[0] = 0.5
        out.append(dict(base, name="item0_too_heavy", means=m3, nfps=w3))
        out.append(dict(base, name="item0_too_heavy_all_zero", means=np.zeros(S, np.float32), nfps=w3))
        w4 = w.copy(); w4[0] = min(int(w4[0]), max(cap, 0))
        out.append(dict(base, name="all_values_zero_item0_fits", means=np.zeros(S, np.float32), nfps=w4))
        k5 = min(S, cap, 48)
        w5 = np.zeros(S, np.int32); w5[:k5] = cap // k5 if cap else 0                               # capacity >= the sum of the weights
        m5 = np.where(w5 > 0, np.float32(0.25), np.float32(0.0)).astype(np.float32)
        assert int(w5.sum()) <= cap
        out.append(dict(base, name="everything_fits", means=m5, nfps=w5))
        out.append(dict(base, name="all_equal", means=np.full(S, 0.25, np.float32), nfps=w))
        out.append(dict(base, name="random", means=rng.standard_normal(S).astype(np.float32), nfps=rng.integers(0, wmax + 1, size=S).astype(np.int32)))
    for i, v in enumerate(out):
        U = (0, 1, 3, 32)[i % 4]
        v["mask"] = (rng.random((U, n_frames)) < 0.3).astype(np.uint8) if U else None
        if U == 3:
            v["mask"][1] = 0                                                                        # an annotator who selected nothing
    return out


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("method", [0, 1])
def test_integer_problems_equal_the_host(method, cap):
    vids = _problems(cap, 900 + cap)
    proportion = 1.0 if cap else 0.5
    assert all(int(np.floor(float(v["n_frames"]) * proportion)) == cap for v in vids)
    got = _select_call(vids, method)
    _check(got, vids, proportion, method, f"cap={cap} method={method}")
    lens = [int(v["nfps"].sum()) for v in vids]
    assert any(L < v["n_frames"] for L, v in zip(lens, vids)) or cap < 2
    assert any(L > v["n_frames"] for L, v in zip(lens, vids)) or cap < 2


# ------------------------------------------------------------------------------------------------ 2. evaluate_batch_device(select="device")
def _prepare(v):
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    return eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"],
                                     E.rank_users(v["user_scores"]))


def _plain_batch():
    """The seven (T, U) videos of tests/test_gpu_evaltail.py with its tie edits, and four more: a summary shorter than the video (the
    float64 F-score branch), one longer than it, a single annotator with a short summary, an annotator who selected nothing."""
    rng = np.random.default_rng(11)
    vids, scores, lens = [], [], []
    for i, (T, U) in enumerate([(300, 15), (1, 3), (97, 20), (650, 18), (33, 5), (320, 32), (150, 1), (120, 4), (120, 4), (80, 1), (200, 6)]):
        v = R.synthetic_video(T, 8100 + i, n_users=U)
        s = rng.random(T).astype(np.float32)
        if i == 2:
            s[10:40] = s[10]
        if i == 4:
            s[:] = 0.25
        nfps = v["n_frame_per_seg"].copy()
        if i in (7, 9):
            nfps[-1] -= 9                                       # sum(nfps) < n_frames
        if i == 8:
            nfps[0] += 11                                       # sum(nfps) > n_frames
        if i == 10:
            v["user_summary"][2] = 0                            # an annotator who selected nothing
        vids.append(_prepare(dict(v, n_frame_per_seg=nfps)))
        scores.append(s); lens.append(T)
    assert sum(int(v["nfps"].sum()) < v["n_frames"] for v in vids) == 2 and sum(int(v["nfps"].sum()) > v["n_frames"] for v in vids) == 1
    return vids, scores, lens


def _compare_with_host(vids, scores, lens, method, metric, want_summaries=True):
    from summarizer_amd.utils import eval_native
    dev = _dev()
    want = eval_native.evaluate_batch(vids, scores, 0.15, method, want_summaries=want_summaries, n_threads=3, metric=metric)
    packed = torch.from_numpy(np.concatenate(scores)).to(dev)
    host = eval_native.evaluate_batch_device(vids, packed, lens, 0.15, method, want_summaries=want_summaries, n_threads=3, metric=metric, select="host")
    got = eval_native.evaluate_batch_device(vids, packed, lens, 0.15, method, want_summaries=want_summaries, metric=metric, select="device")
    np.testing.assert_array_equal(got[0], host[0])                           # the correlation kernels and their inputs are the same
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(host[1], want[1])
    if want_summaries:
        assert len(got[3]) == len(want[3])
        for a, b in zip(got[3], want[3]):
            assert a.dtype == np.float32
            np.testing.assert_array_equal(a, b)
    else:
        assert got[3] is None
    return got


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
@pytest.mark.parametrize("method", ["knapsack", "rank"])
def test_batch_select_on_device_equals_host_tail(method, metric):
    from summarizer_amd.utils import eval_native
    vids, scores, lens = _plain_batch()
    assert all(eval_native.select_device_ready(v, 0.15) for v in vids)
    first = _compare_with_host(vids, scores, lens, method, metric)
    assert np.isfinite(first[1]).all() and np.isfinite(first[2]).all()
    # the cached batch with other scores, then a sub-batch of it
    rng = np.random.default_rng(12)
    scores2 = [rng.random(T).astype(np.float32) for T in lens]
    second = _compare_with_host(vids, scores2, lens, method, metric, want_summaries=False)
    assert not np.array_equal(second[0], first[0])
    sub = [0, 3, 5, 7, 8]
    _compare_with_host([vids[i] for i in sub], [scores2[i] for i in sub], [lens[i] for i in sub], method, metric)
    ent = eval_native._DEV_BATCH_CACHE[(tuple(id(v) for v in vids), tuple(lens), str(_dev()))]
    assert (0.15, eval_native.METHODS[method]) in ent["select"] and "mask" in vids[0]["_dev"][str(_dev())]


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
@pytest.mark.parametrize("method", ["knapsack", "rank"])
def test_edge_batch_select_on_device_equals_host_tail(method, metric):
    from summarizer_amd.utils import eval_native
    batch = R.eval_edge_batch()
    vids = [_prepare(v) for _, v, _ in batch]
    scores, lens = [s for _, _, s in batch], [v["n_steps"] for _, v, _ in batch]
    assert all(eval_native.select_device_ready(v, 0.15) and eval_native.kendall_device_ready(v) for v in vids)
    _compare_with_host(vids, scores, lens, method, metric)
    # the same bits with every device buffer of the select side poisoned
    dev = _dev()
    ent = eval_native._DEV_BATCH_CACHE[(tuple(id(v) for v in vids), tuple(lens), str(dev))]
    se = ent["select"][(0.15, eval_native.METHODS[method])]
    for k in ("summary", "selected", "res", "ws"):
        se[k].view(torch.uint8).fill_(255)
    _compare_with_host(vids, scores, lens, method, metric)


def test_select_argument_and_readiness_are_checked():
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    v = _prepare(R.synthetic_video(60, 8200, n_users=4))
    s = torch.zeros(60, device=_dev())
    with pytest.raises(KeyError):
        eval_native.evaluate_batch_device([v], s, [60], select="gpu")
    with pytest.raises(_lib.SumkError, match="select"):
        eval_native.evaluate_batch_device([v], s, [60], proportion=10.0, select="device")          # a budget of 8910 frames


# ------------------------------------------------------------------------------------------------ 3. poison / 4. refusals
def _three_videos(seed=5):
    rng = np.random.default_rng(seed)
    vids = []
    for S, n_frames, U in ((12, 400, 3), (40, 900, 1), (7, 150, 5)):
        w = rng.multinomial(n_frames, np.ones(S) / S).astype(np.int32)
        vids.append(dict(means=rng.choice(np.array([0.0, 0.25, 0.5, 0.75], np.float32), size=S), nfps=w, n_frames=n_frames,
                         capacity=int(np.floor(n_frames * 0.15)), mask=(rng.random((U, n_frames)) < 0.2).astype(np.uint8)))
    return vids


@pytest.mark.parametrize("method", [0, 1])
def test_poisoned_buffers_and_gaps(method):
    """Every output and the workspace start as 0xFF bytes (always, in _select_call); the results are the host's, two calls agree bit for
    bit, and the entries of machine_summary between the videos' ranges -- 17 apart here -- are still 0xFF afterwards."""
    vids = _three_videos()
    a = _select_call(vids, method, gap=17)
    _check(a, vids, 0.15, method)
    assert a["outside"].sum() == 4 * 17
    b = _select_call(vids, method, gap=17)
    assert np.array_equal(a["raw"].view(np.uint32), b["raw"].view(np.uint32)) and np.array_equal(a["raw_selected"], b["raw_selected"])
    assert np.array_equal(a["f_avg"].view(np.uint64), b["f_avg"].view(np.uint64)) and np.array_equal(a["f_max"].view(np.uint64), b["f_max"].view(np.uint64))


def test_refusals_launch_nothing():
    from summarizer_amd.utils import eval_native
    rng = np.random.default_rng(6)

    def untouched(r):
        assert r["rc"] == -1, r["rc"]                                        # SUMK_ERR_ARG
        assert (r["raw"].view(np.uint32) == 0xFFFFFFFF).all() and (r["raw_selected"] == 255).all()
        assert (r["status"] == -1).all() and (r["f_avg"].view(np.uint64) == 2 ** 64 - 1).all() and (r["f_max"].view(np.uint64) == 2 ** 64 - 1).all()

    good = _three_videos()
    # one segment over the limit (the descriptor says 1025; the buffers hold 1025)
    big = dict(means=np.zeros(1025, np.float32), nfps=np.ones(1025, np.int32), n_frames=1025, capacity=153, mask=None)
    r = _select_call([good[0], big], 0)
    untouched(r); assert "1025 segments" in r["error"]
    assert eval_native.select_refusal(1025, 1025, 0, 0.15) is not None and eval_native.select_refusal(1024, 1025, 0, 0.15) is None
    # one annotator over the limit
    crowd = dict(good[1], mask=(rng.random((33, good[1]["n_frames"])) < 0.2).astype(np.uint8))
    r = _select_call([crowd, good[2]], 1)
    untouched(r); assert "33 annotators" in r["error"]
    assert eval_native.select_refusal(40, 900, 33, 0.15) is not None and eval_native.select_refusal(40, 900, 32, 0.15) is None
    # a workspace one byte short
    r = _select_call(good, 0, ws_short=1)
    untouched(r); assert "workspace" in r["error"]
    # and the call goes through with the byte back
    _check(_select_call(good, 0), good, 0.15, 0)


@pytest.mark.parametrize("method", [0, 1])
def test_non_finite_segment_mean_gives_status_1_there_only(method):
    good = _three_videos(8)
    for poison in (np.float32("nan"), np.float32("inf"), np.float32(-3e12)):
        vids = [dict(v) for v in good]
        vids[1] = dict(vids[1], means=vids[1]["means"].copy())
        vids[1]["means"][5] = poison
        r = _select_call(vids, method, gap=5)
        assert r["rc"] == 0 and r["status"].tolist() == [0, 1, 0]
        assert (r["summaries"][1] == 0).all() and (r["selected"][1] == 0).all() and np.isnan(r["f_avg"][1]) and np.isnan(r["f_max"][1])
        assert (r["raw"][r["outside"]].view(np.uint32) == 0xFFFFFFFF).all()
        alone = _select_call([good[0], good[2]], method)
        _check(alone, [good[0], good[2]], 0.15, method)
        for i, j in ((0, 0), (2, 1)):
            np.testing.assert_array_equal(r["summaries"][i], alone["summaries"][j])
            np.testing.assert_array_equal(r["selected"][i], alone["selected"][j])
            assert r["f_avg"][i] == alone["f_avg"][j] and r["f_max"][i] == alone["f_max"][j]


def _given_up(r, i, status, good, method, written=True):
    """Video i of call r was given up with `status`: an all-zero summary and selection (written=False: neither was written), NaN
    F-scores; its neighbours -- `good` without video i gives them alone -- are what they are without it; nothing else was touched."""
    assert r["rc"] == 0, r["error"]
    assert r["status"].tolist() == [status if j == i else 0 for j in range(len(good))]
    if written:
        assert (r["summaries"][i] == 0).all() and (r["selected"][i] == 0).all()
    else:
        assert (r["summaries"][i].view(np.uint32) == 0xFFFFFFFF).all() and (r["selected"][i] == 255).all()
    assert np.isnan(r["f_avg"][i]) and np.isnan(r["f_max"][i])
    assert (r["raw"][r["outside"]].view(np.uint32) == 0xFFFFFFFF).all()
    others = [j for j in range(len(good)) if j != i]
    alone = _select_call([good[j] for j in others], method)
    _check(alone, [good[j] for j in others], 0.15, method)
    for k, j in enumerate(others):
        np.testing.assert_array_equal(r["summaries"][j], alone["summaries"][k])
        np.testing.assert_array_equal(r["selected"][j], alone["selected"][k])
        assert r["f_avg"][j] == alone["f_avg"][k] and r["f_max"][j] == alone["f_max"][k]


def test_values_past_the_int32_rows_give_status_2_in_knapsack_mode_only():
    """1024 segments of mean 3000: each value 3e6, together 3.07e9 >= 2^31.  The knapsack gives the video up (status 2); the rank walk has
    no profit rows and equals the host."""
    good = _three_videos(9)
    rng = np.random.default_rng(10)
    n_frames = 4000
    big = dict(means=np.full(1024, 3000.0, np.float32), nfps=rng.integers(1, 9, size=1024).astype(np.int32), n_frames=n_frames,
               capacity=int(np.floor(n_frames * 0.15)), mask=(rng.random((2, n_frames)) < 0.2).astype(np.uint8))
    vids = [good[0], big, good[2]]
    _given_up(_select_call(vids, 0, gap=5), 1, 2, vids, 0)
    _check(_select_call(vids, 1), vids, 0.15, 1)
    # just below: 1024 x 2 097 000 = 2 147 328 000 < 2^31 -- the host's result
    vids[1] = dict(big, means=np.full(1024, 2097.0, np.float32))
    assert 1024 * 2097000 < 2 ** 31
    _check(_select_call(vids, 0), vids, 0.15, 0)


@pytest.mark.parametrize("method", [0, 1])
def test_nfps_that_disagree_with_summary_len_give_status_3(method):
    good = _three_videos(12)
    for delta in (-1, 1):                          # summary_len one short of / one past the sum of nfps
        r = _select_call(good, method, gap=5, override={1: dict(summary_len=int(good[1]["nfps"].sum()) + delta)})
        _given_up(r, 1, 3, good, method)
    neg = [dict(v) for v in good]
    neg[2] = dict(neg[2], nfps=neg[2]["nfps"].copy())
    neg[2]["nfps"][3] = -2
    _given_up(_select_call(neg, method, gap=5), 2, 3, good, method)


def test_a_device_descriptor_past_the_limits_gives_status_4_and_writes_nothing_else():
    """The entry point checks the host copy; a device copy that disagrees (1025 segments, a budget of 8192, 33 annotators) is given up by
    its workgroup before it touches LDS, the workspace or its outputs."""
    good = _three_videos(13)
    for fields in (dict(n_segs=1025), dict(capacity=8192), dict(n_users=33), dict(method=2)):
        _given_up(_select_call(good, 0, gap=5, dev_override={0: fields}), 0, 4, good, 0, written=False)


# ------------------------------------------------------------------------------------------------ 5. pad segments
@pytest.mark.parametrize("method", [0, 1])
def test_empty_pad_segments_change_nothing(method):
    rng = np.random.default_rng(31)
    live, padded = [], []
    for S, n_frames in ((9, 700), (30, 2000), (1, 90)):
        w = rng.multinomial(n_frames, np.ones(S) / S).astype(np.int32)
        m = rng.choice(np.array([0.0, 0.0, 0.25, 0.5], np.float32), size=S)          # ties at the pads' own mean, 0
        mask = (rng.random((4, n_frames)) < 0.2).astype(np.uint8)
        v = dict(means=m, nfps=w, n_frames=n_frames, capacity=int(np.floor(n_frames * 0.15)), mask=mask)
        live.append(v)
        padded.append(dict(v, means=np.concatenate([m, np.zeros(1024 - S, np.float32)]), nfps=np.concatenate([w, np.zeros(1024 - S, np.int32)])))
    a, b = _select_call(live, method), _select_call(padded, method)
    _check(a, live, 0.15, method); _check(b, padded, 0.15, method)
    for i in range(3):
        np.testing.assert_array_equal(a["summaries"][i], b["summaries"][i])
    np.testing.assert_array_equal(a["f_avg"], b["f_avg"]); np.testing.assert_array_equal(a["f_max"], b["f_max"])


def test_kts_segments_kernel_equals_the_numpy_layout():
    from summarizer_amd import kernels
    from summarizer_amd.utils import kts
    dev = _dev()
    rng = np.random.default_rng(41)
    lens, max_ncp = [40, 1, 2, 130, 300], 20
    n_cps = np.array([3, 0, 1, 20, 0], np.int32)
    cps = np.full((5, max_ncp), -1, np.int32)
    for v, n in enumerate(lens):
        cps[v, :n_cps[v]] = np.sort(rng.choice(np.arange(1, n), size=n_cps[v], replace=False)) if n_cps[v] else []
    picks = [None, None, np.array([0, 9], np.int32), (3 * np.arange(130)).astype(np.int32), None]
    n_frames = [40, 1, 20, 395, 300]
    pk_dev = [torch.from_numpy(p).to(dev) if p is not None else None for p in picks]
    ptrs = torch.tensor([t.data_ptr() if t is not None else 0 for t in pk_dev], dtype=torch.int64, device=dev)
    sb = kernels.SeqBatch.get(lens, dev)
    cp, nfps = kernels.kts_segments(torch.from_numpy(n_cps).to(dev), torch.from_numpy(cps).to(dev), sb, ptrs, torch.tensor(n_frames, dtype=torch.int32, device=dev))
    cp0, nfps0 = kernels.kts_segments(torch.from_numpy(n_cps).to(dev), torch.from_numpy(cps).to(dev), sb, None, torch.tensor(lens, dtype=torch.int32, device=dev))
    cp, nfps, cp0, nfps0 = cp.cpu().numpy(), nfps.cpu().numpy(), cp0.cpu().numpy(), nfps0.cpu().numpy()
    for v, n in enumerate(lens):
        want = kts.cps_to_segments_padded(cps[v, :n_cps[v]], np.arange(n) if picks[v] is None else picks[v], n_frames[v], max_ncp + 1)
        np.testing.assert_array_equal(cp[v], want[0]); np.testing.assert_array_equal(nfps[v], want[1])
        want0 = kts.cps_to_segments_padded(cps[v, :n_cps[v]], np.arange(n), n, max_ncp + 1)
        np.testing.assert_array_equal(cp0[v], want0[0]); np.testing.assert_array_equal(nfps0[v], want0[1])


# ------------------------------------------------------------------------------------------------ 6. Summarizer(device=True)
@pytest.mark.parametrize("method", ["knapsack", "rank"])
def test_summarizer_on_device_equals_the_default(method, monkeypatch):
    import summarizer_amd
    from summarizer_amd import _lib
    from summarizer_amd.models.vasnet import VASNet
    from summarizer_amd.utils import eval_native
    dev = _dev()
    torch.manual_seed(5)
    model = VASNet(input_size=64).eval().to(dev)
    lens = [40, 1, 2, 130, 300]
    feats = [torch.from_numpy(R.features(T, 1, 64, 300 + T)[:, 0, :].copy()).to(dev) for T in lens]
    picks = [None, None, None, (4 * np.arange(130) + 2).astype(np.int32), None]
    n_frames = [None, None, None, 4 * 130 + 3, None]
    host = summarizer_amd.Summarizer(model, proportion=0.3, method=method).summarize_batch(feats, picks, n_frames)
    ondev = summarizer_amd.Summarizer(model, proportion=0.3, method=method, device=True).summarize_batch(feats, picks, n_frames)
    assert len(ondev) == len(host) == 5
    some_cps = 0
    for h, d in zip(host, ondev):
        assert all(torch.is_tensor(d[k]) and d[k].is_cuda for k in ("scores", "machine_summary", "change_points", "n_frame_per_seg", "n_segs", "status"))
        S = int(d["n_segs"])
        assert S == h["change_points"].shape[0] and int(d["status"]) == 0
        some_cps += S - 1
        np.testing.assert_array_equal(d["scores"].cpu().numpy(), h["scores"])
        np.testing.assert_array_equal(d["change_points"].cpu().numpy()[:S], h["change_points"])
        np.testing.assert_array_equal(d["n_frame_per_seg"].cpu().numpy()[:S], h["n_frame_per_seg"])
        assert (d["n_frame_per_seg"].cpu().numpy()[S:] == 0).all()
        np.testing.assert_array_equal(d["machine_summary"].cpu().numpy(), h["machine_summary"])
        assert d["machine_summary"].dtype == torch.float32
    assert some_cps > 0 and any(h["machine_summary"].sum() > 0 for h in host)
    # past the limit: the predicate's limit patched down, not a huge input
    monkeypatch.setattr(eval_native, "SELECT_MAX_CAPACITY", 50)
    with pytest.raises(_lib.SumkError, match="budget of"):
        summarizer_amd.Summarizer(model, proportion=0.3, method=method, device=True).summarize_batch(feats, picks, n_frames)
    monkeypatch.undo()
    with pytest.raises(_lib.SumkError, match="ascend"):
        summarizer_amd.Summarizer(model, device=True).summarize(feats[0], picks=np.arange(40)[::-1].copy(), n_frames=40)
    # one pick over the device tail's 4096: refused before anything is scored (4096 itself passes the check and fails on the next one)
    with pytest.raises(_lib.SumkError, match="4097 picks"):
        summarizer_amd.Summarizer(model, device=True, max_ncp=5).summarize(torch.zeros(4097, 64, device=dev))
    with pytest.raises(_lib.SumkError, match="ascend"):
        summarizer_amd.Summarizer(model, device=True, max_ncp=5).summarize(torch.zeros(4096, 64, device=dev), picks=np.arange(4096)[::-1].copy())


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_segments_and_select_replay_from_a_graph():
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    lib, dev = _lib.load(), _dev()
    rng = np.random.default_rng(51)
    raw = [R.synthetic_video(T, 8500 + i, n_users=U) for i, (T, U) in enumerate([(120, 3), (45, 1), (200, 7)])]
    vids, lens, n = [_prepare(v) for v in raw], [120, 45, 200], 3
    vd, sd = (_lib.EvalDevVideo * n)(), (_lib.EvalDevSelect * n)()
    metas = [eval_native._device_meta(v, dev, select=True) for v in vids]
    segs, frames = sum(v["cps"].shape[0] for v in vids), sum(v["n_frames"] for v in vids)
    scores = torch.zeros(sum(lens), dtype=torch.float32, device=dev)
    seg, scratch = _poisoned(segs, torch.float32, dev), _poisoned(frames, torch.float32, dev)
    total = sum(int(v["nfps"].sum()) for v in vids)
    summary, selected = _poisoned(total, torch.float32, dev), _poisoned(segs, torch.uint8, dev)
    f, status = _poisoned(2 * n, torch.float64, dev), _poisoned(n, torch.int32, dev)
    row0 = frame0 = seg0 = at = 0
    for i, (v, m, T) in enumerate(zip(vids, metas, lens)):
        e, q = vd[i], sd[i]
        e.picks, e.n_picks, e.n_frames, e.n_steps, e.row0, e.frame0 = m["picks"].data_ptr(), v["picks"].shape[0], v["n_frames"], T, row0, frame0
        e.cps, e.n_segs, e.seg0 = m["cps"].data_ptr(), v["cps"].shape[0], seg0
        q.seg_means, q.nfps, q.n_segs, q.n_frames = seg.data_ptr() + 4 * seg0, m["nfps"].data_ptr(), v["cps"].shape[0], v["n_frames"]
        q.capacity, q.summary_len, q.summary0, q.sel0 = eval_native.select_capacity(v["n_frames"], 0.15), int(v["nfps"].sum()), at, seg0
        q.user_mask, q.n_users, q.method = m["mask"].data_ptr(), m["mask"].shape[0], 0
        row0 += T; frame0 += v["n_frames"]; seg0 += v["cps"].shape[0]; at += q.summary_len
    vd_dev = torch.frombuffer(bytearray(bytes(vd)), dtype=torch.uint8).to(dev)
    sd_dev = torch.frombuffer(bytearray(bytes(sd)), dtype=torch.uint8).to(dev)
    ws = _poisoned(lib.sumk_eval_device_select_workspace_bytes(n, max(q.n_segs for q in sd), max(q.capacity for q in sd)), torch.uint8, dev)

    def enqueue():
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.sumk_eval_device_segments(scores.data_ptr(), vd_dev.data_ptr(), n, scratch.data_ptr(), seg.data_ptr(), st), "segments")
        _lib.check(lib.sumk_eval_device_select(sd_dev.data_ptr(), C.cast(sd, C.c_void_p), n, summary.data_ptr(), total, selected.data_ptr(), segs,
                                               f.data_ptr(), f.data_ptr() + 8 * n, status.data_ptr(), ws.data_ptr(), ws.numel(), st), "select")
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                    # one capture stream, the two launches in order: a linear graph
        enqueue()
    for rep in range(2):
        s = [rng.random(T).astype(np.float32) for T in lens]
        scores.copy_(torch.from_numpy(np.concatenate(s)).to(dev))
        for t in (summary, selected, f, status, ws, seg):
            t.view(torch.uint8).fill_(255)
        g.replay()
        torch.cuda.synchronize(dev)
        want = eval_native.evaluate_batch(vids, s, 0.15, "knapsack", want_summaries=True, n_threads=2)
        assert status.cpu().tolist() == [0, 0, 0]
        np.testing.assert_array_equal(f.cpu().numpy()[:n], want[1]); np.testing.assert_array_equal(f.cpu().numpy()[n:], want[2])
        np.testing.assert_array_equal(summary.cpu().numpy(), np.concatenate(want[3]))


# ------------------------------------------------------------------------------------------------ 8. Trainer opt-in
def _trainer(ds, keys, **over):
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.hps import make_hps
    hps = make_hps(ds, [{"train_keys": [], "test_keys": keys}], epochs=1, extra_params={"input_size": "128"}, **over)
    torch.manual_seed(77)
    return VASNetTrainer(hps, hps.splits_files[0]).reset()


@pytest.mark.parametrize("algorithm", ["knapsack", "rank"])
def test_trainer_selection_device_returns_the_same_tuple(algorithm, monkeypatch):
    from summarizer_amd.utils import eval_native
    from summarizer_amd.utils.datasets import synthetic_dataset
    ds = synthetic_dataset(6, seed=41, D=128, t_range=(30, 90), n_users=5)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
    default = _trainer(ds, keys, selection_algorithm=algorithm).test(0)
    calls = []
    real = eval_native.evaluate_batch_device
    monkeypatch.setattr(eval_native, "evaluate_batch_device", lambda *a, **k: (calls.append(k.get("select")), real(*a, **k))[1])
    opted = _trainer(ds, keys, selection_algorithm=algorithm, selection_device=True).test(0)
    assert calls == ["device"]
    assert opted[0] == default[0] and opted[1][0] == default[1][0] and opted[1][1] == default[1][1]
    assert np.isfinite(opted[0]) and np.isfinite(opted[1][0])
    # a video past the predicate: today's path, the same numbers
    monkeypatch.setattr(eval_native, "SELECT_MAX_SEGS", 1)
    calls.clear()
    again = _trainer(ds, keys, selection_algorithm=algorithm, selection_device=True).test(0)
    assert calls == ["host"] and again[0] == default[0] and again[1] == default[1]


def test_trainer_falls_back_to_the_host_tail_on_a_device_status(monkeypatch):
    """What only the device sees (SelectStatusError) does not reach the caller of Trainer.test: the host tail gives the batch's numbers."""
    from summarizer_amd.utils import eval_native
    from summarizer_amd.utils.datasets import synthetic_dataset
    ds = synthetic_dataset(4, seed=43, D=128, t_range=(30, 60), n_users=3)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
    default = _trainer(ds, keys).test(0)
    calls = []
    real = eval_native.evaluate_batch_device

    def flaky(*a, **k):
        calls.append(k.get("select"))
        if k.get("select") == "device":
            raise eval_native.SelectStatusError("video 0: status 1")
        return real(*a, **k)
    monkeypatch.setattr(eval_native, "evaluate_batch_device", flaky)
    opted = _trainer(ds, keys, selection_device=True).test(0)
    assert calls == ["device", "host"] and opted[0] == default[0] and opted[1] == default[1]


def test_batch_api_raises_select_status_error_on_a_nan_score():
    """A NaN score makes a NaN segment mean: select="device" raises SelectStatusError (a SumkError) naming the video."""
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    vids = [_prepare(R.synthetic_video(T, 8600 + i, n_users=2)) for i, T in enumerate((40, 50))]
    s = np.linspace(0, 1, 90, dtype=np.float32)
    s[60] = np.nan
    assert issubclass(eval_native.SelectStatusError, _lib.SumkError)
    with pytest.raises(eval_native.SelectStatusError, match="video 1"):
        eval_native.evaluate_batch_device(vids, torch.from_numpy(s).to(_dev()), [40, 50], select="device")
