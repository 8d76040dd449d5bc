"""GPU: the evaluation tail for long videos (csrc/evallong.hip: sumk_eval_device_segments_long, sumk_eval_device_select_long) and
`Summarizer(device=True, tail="long")`.

The references are the host tail -- `sumk_eval_videos` with the segment means given, `sumk_knapsack_dp`, numpy's `upsample` and float32
`.mean()` -- and, wherever their limits admit the input, the one-workgroup kernels `sumk_eval_device_select` / `sumk_eval_device_segments`.
Every comparison is `assert_array_equal`: integers, float32 sums in numpy's order and integer F-score counts leave nothing to tolerate.  All
output and workspace buffers start as 0xFF bytes (the helpers follow tests/test_gpu_select.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 2048             # SUMK_SELECT_LONG_CHUNK: capacities per block of a DP launch
OLD_MAX_CAP = 8191       # SUMK_SELECT_MAX_CAPACITY: the largest budget sumk_eval_device_select takes
OLD_MAX_INT = 4096       # ED_MAX_INT: the most pick intervals sumk_eval_device_segments takes


def _dev():
    return torch.device("cuda:0")


def _poisoned(numel, dtype, dev):
    t = torch.empty(max(int(numel), 1), dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(255)
    return t


# ------------------------------------------------------------------------------------------------ helpers: select
def _select_call(vids, method, gap=3, ws_short=0, override=None, dev_override=None, entry="long", null=(), totals=None):
    """sumk_eval_device_select_long (entry="block": sumk_eval_device_select) on buffers of the test's own, all of them -- the workspace
    too -- filled with 0xFF bytes first.  vids: dicts with means (S,) float32, nfps (S,) int32, n_frames, capacity and mask (U, n_frames)
    uint8 or None; the videos' ranges in the summary buffer are `gap` entries apart.  override: {video: {field: value}} on the HOST AND
    DEVICE copy of the descriptors; dev_override: the same on the device copy alone (what the entry point cannot see); null: arguments
    passed as null pointers; totals: (summary_total, selected_total) told to the call instead of the buffers' sizes."""
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
        ranges.append((at, at + e.summary_len))
        at += e.summary_len + gap; seg_at += S
        for k, val in (override or {}).get(i, {}).items():
            setattr(e, k, val)
    on_dev = (_lib.EvalDevSelect * n).from_buffer_copy(bytes(descr))
    for i, fields in (dev_override or {}).items():
        for k, val in fields.items():
            setattr(on_dev[i], k, val)
    descr_dev = torch.frombuffer(bytearray(bytes(on_dev)), dtype=torch.uint8).to(dev)
    max_segs, max_cap = max(len(v["means"]) for v in vids), max(int(v["capacity"]) for v in vids)
    size_of = lib.sumk_eval_device_select_long_workspace_bytes if entry == "long" else lib.sumk_eval_device_select_workspace_bytes
    ws_bytes = size_of(n, min(max_segs, 1024), min(max(max_cap, 0), 1 << 24))
    assert ws_bytes > 0
    summary, selected = _poisoned(at, torch.float32, dev), _poisoned(seg_at, torch.uint8, dev)
    f_avg, f_max, status = _poisoned(n, torch.float64, dev), _poisoned(n, torch.float64, dev), _poisoned(n, torch.int32, dev)
    ws = _poisoned(ws_bytes, torch.uint8, dev)
    call = lib.sumk_eval_device_select_long if entry == "long" else lib.sumk_eval_device_select
    ptr = dict(descr_dev=descr_dev.data_ptr(), descr=C.cast(descr, C.c_void_p), summary=summary.data_ptr(), selected=selected.data_ptr(),
               f_avg=f_avg.data_ptr(), f_max=f_max.data_ptr(), status=status.data_ptr(), ws=ws.data_ptr())
    for k in null:
        ptr[k] = None
    s_total, sel_total = totals if totals is not None else (at, seg_at)
    rc = call(ptr["descr_dev"], ptr["descr"], n, ptr["summary"], s_total, ptr["selected"], sel_total, ptr["f_avg"], ptr["f_max"], ptr["status"],
              ptr["ws"], ws_bytes - ws_short, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
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
    assert all(int(np.floor(float(v["n_frames"]) * proportion)) == v["capacity"] for v in vids), what
    summaries, f_avg, f_max = _host_tail(vids, proportion, method)
    for i, v in enumerate(vids):
        np.testing.assert_array_equal(got["selected"][i], _expected_selected(v, method), err_msg=f"{what} video {i} ({v.get('name')})")
        np.testing.assert_array_equal(got["summaries"][i], summaries[i], err_msg=f"{what} video {i} ({v.get('name')})")
    np.testing.assert_array_equal(got["f_avg"], f_avg, err_msg=what)
    np.testing.assert_array_equal(got["f_max"], f_max, err_msg=what)
    assert (got["raw"][got["outside"]].view(np.uint32) == 0xFFFFFFFF).all(), what          # nothing written outside the videos' ranges


def _same_results(a, b, pairs, what=""):
    """Videos (i of call a, j of call b) have the same bits in every output."""
    for i, j in pairs:
        np.testing.assert_array_equal(a["summaries"][i], b["summaries"][j], err_msg=what)
        np.testing.assert_array_equal(a["selected"][i], b["selected"][j], err_msg=what)
        np.testing.assert_array_equal(a["f_avg"][i:i + 1].view(np.uint64), b["f_avg"][j:j + 1].view(np.uint64), err_msg=what)
        np.testing.assert_array_equal(a["f_max"][i:i + 1].view(np.uint64), b["f_max"][j:j + 1].view(np.uint64), err_msg=what)
        assert a["status"][i] == b["status"][j], what


# ------------------------------------------------------------------------------------------------ 1. integer problems through the C entry
SEGS = (1, 2, 64, 65, 1024)
# capacity + 1 in {1, 2, 64, 65}; the last capacity of a DP block, the first of the next and one more; the LDS threshold of the
# one-workgroup kernel; its limit and past it; ten DP blocks
CAPS = (0, 1, 63, 64, CHUNK - 1, CHUNK, CHUNK + 1, 4095, 4096, 8191, 8192, 8193, 20000)


def _problems(cap, seed):
    """One budget, every segment count, the contents that decide ties and quirks (the recipe of tests/test_gpu_select.py).  n_frames = the
    budget (proportion 1; budget 0: one frame at proportion 0.5), so summaries are shorter than, equal to and longer than the video: both
    F-score branches."""
    rng = np.random.default_rng(seed)
    n_frames = max(cap, 1)
    out = []
    for S in SEGS:
        wmax = max(1, cap // 3)
        tied = rng.choice(np.array([0.0, 0.25, 0.5], np.float32), size=S)
        # (weights in the upper half of [1, budget / 3]: a handful of key shots per video, so the host reference, which re-solves its
        #  DP once per selected item, stays quick at 1024 segments x 20 001 capacities; small budgets leave many EQUAL weights: tied optima)
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
def test_integer_problems_equal_the_host_and_the_block_kernel(method, cap):
    vids = _problems(cap, 1900 + cap)
    proportion = 1.0 if cap else 0.5
    got = _select_call(vids, method)
    _check(got, vids, proportion, method, f"cap={cap} method={method}")
    assert {0, 1, 3, 32} == {0 if v["mask"] is None else v["mask"].shape[0] for v in vids}
    lens = [int(v["nfps"].sum()) for v in vids]
    assert any(L < v["n_frames"] for L, v in zip(lens, vids)) or cap < 2
    assert any(L > v["n_frames"] for L, v in zip(lens, vids)) or cap < 2
    if cap <= OLD_MAX_CAP:
        block = _select_call(vids, method, entry="block")
        assert block["rc"] == 0, block["error"]
        _same_results(got, block, [(i, i) for i in range(len(vids))], f"cap={cap} method={method} against sumk_eval_device_select")


# ------------------------------------------------------------------------------------------------ 2. one call, many kinds of video
def _mixed_videos():
    """Budgets 0, 60, 600, 2048 (= CHUNK: two DP blocks, the second with one capacity) and 9000 at proportion 0.15; 1 .. 1024 segments with
    5 .. 1024 of them in the pass; video 2 is given up in knapsack mode (its values pass the int32 profit rows: status 2)."""
    rng = np.random.default_rng(77)
    geo = ((12, 400, 3), (5, 6, 2), (1024, 4000, 2), (40, 60000, 1), (1024, 13654, 4), (1, 90, 0), (300, 4000, 32))
    vids = []
    for i, (S, n_frames, U) in enumerate(geo):
        cap = int(np.floor(n_frames * 0.15))
        if i == 2:
            means, w = np.full(S, 3000.0, np.float32), rng.integers(1, 9, size=S).astype(np.int32)
        elif i == 4:
            means = rng.choice(np.array([0.0, 0.0, 0.0, 0.25, 0.5], np.float32), size=S)
            w = rng.integers(cap // 6, cap // 3, size=S).astype(np.int32)
        else:
            means = rng.choice(np.array([0.0, 0.25, 0.5, 0.75], np.float32), size=S)
            w = rng.multinomial(n_frames, np.ones(S) / S).astype(np.int32)
        vids.append(dict(means=means, nfps=w, n_frames=n_frames, capacity=cap, mask=(rng.random((U, n_frames)) < 0.2).astype(np.uint8) if U else None))
    assert [v["capacity"] for v in vids] == [60, 0, 600, 9000, CHUNK, 13, 600]
    return vids


@pytest.mark.parametrize("method", [0, 1])
def test_mixed_batch_videos_do_not_touch_each_other(method):
    vids = _mixed_videos()
    r = _select_call(vids, method, gap=17)
    assert r["rc"] == 0, r["error"]
    given_up = [2] if method == 0 else []
    assert r["status"].tolist() == [2 if i in given_up else 0 for i in range(len(vids))]
    for i in given_up:
        assert (r["summaries"][i] == 0).all() and (r["selected"][i] == 0).all() and np.isnan(r["f_avg"][i]) and np.isnan(r["f_max"][i])
    assert (r["summaries"][1] == 0).all() and (r["selected"][1] == 0).all()                     # budget 0: nothing selected, F-scores of an empty summary
    healthy = [i for i in range(len(vids)) if i not in given_up]
    alone = _select_call([vids[i] for i in healthy], method)
    _check(alone, [vids[i] for i in healthy], 0.15, method, f"method={method}")
    _same_results(r, alone, [(i, k) for k, i in enumerate(healthy)])
    assert r["outside"].sum() == (len(vids) + 1) * 17
    assert (r["raw"][r["outside"]].view(np.uint32) == 0xFFFFFFFF).all()
    # every video on its own: the same bits (a video's DP launches do not depend on the call's largest budget or segment count)
    for i in (0, 3, 4):
        _same_results(r, _select_call([vids[i]], method), [(i, 0)], f"video {i} alone")
    # two calls agree bit for bit
    again = _select_call(vids, method, gap=17)
    assert np.array_equal(r["raw"].view(np.uint32), again["raw"].view(np.uint32)) and np.array_equal(r["raw_selected"], again["raw_selected"])


@pytest.mark.parametrize("method", [0, 1])
def test_status_1_and_3_are_given_up_alone(method):
    rng = np.random.default_rng(78)
    good = _mixed_videos()[:1] + _mixed_videos()[3:5]
    bad_mean = dict(good[1], means=good[1]["means"].copy()); bad_mean["means"][5] = np.float32("nan")
    r = _select_call([good[0], bad_mean, good[2]], method, gap=5)
    assert r["rc"] == 0 and r["status"].tolist() == [0, 1, 0]
    assert (r["summaries"][1] == 0).all() and (r["selected"][1] == 0).all() and np.isnan(r["f_avg"][1]) and np.isnan(r["f_max"][1])
    neg = dict(good[2], nfps=good[2]["nfps"].copy()); neg["nfps"][int(rng.integers(0, 1024))] = -2
    r3 = _select_call([good[0], good[1], neg], method, gap=5)
    assert r3["rc"] == 0 and r3["status"].tolist() == [0, 0, 3]
    assert (r3["summaries"][2] == 0).all() and (r3["selected"][2] == 0).all() and np.isnan(r3["f_avg"][2])
    off = _select_call(good, method, gap=5, override={1: dict(summary_len=int(good[1]["nfps"].sum()) - 1)})
    assert off["rc"] == 0 and off["status"].tolist() == [0, 3, 0]
    alone = _select_call(good, method)
    _check(alone, good, 0.15, method)
    _same_results(r, alone, [(0, 0), (2, 2)]); _same_results(r3, alone, [(0, 0), (1, 1)]); _same_results(off, alone, [(0, 0), (2, 2)])
    for q in (r, r3, off):
        assert (q["raw"][q["outside"]].view(np.uint32) == 0xFFFFFFFF).all()


# ------------------------------------------------------------------------------------------------ 3. counts past 16 bits and one block
@pytest.mark.parametrize("method", [0, 1])
def test_300000_frames_32_annotators(method):
    """Every count of the F-scores passes 65 535 and no single block sees the video; video 0's summary is shorter than the video (the
    float64 branch), video 1's longer (float32, truncation)."""
    rng = np.random.default_rng(79)
    n_frames, S = 300000, 50
    vids = []
    for delta in (-9, 11):
        w = rng.multinomial(n_frames + delta, np.ones(S) / S).astype(np.int32)
        mask = (rng.random((32, n_frames)) < 0.4).astype(np.uint8)
        mask[3] = 1; mask[7] = 0                                     # selected every frame / selected none
        vids.append(dict(means=rng.random(S).astype(np.float32), nfps=w, n_frames=n_frames, capacity=45000, mask=mask))
    got = _select_call(vids, method, gap=5)
    _check(got, vids, 0.15, method)
    assert all((v["mask"].sum(axis=1)[[0, 3]] > 65535).all() and v["mask"][7].sum() == 0 for v in vids)
    assert all(s.sum() > 0 for s in got["summaries"])
    assert np.isfinite(got["f_avg"]).all() and (got["f_max"] > 0).all()


# ------------------------------------------------------------------------------------------------ 4. error paths
def _untouched(r):
    assert r["rc"] == -1, r["rc"]                                        # SUMK_ERR_ARG
    assert (r["raw"].view(np.uint32) == 0xFFFFFFFF).all() and (r["raw_selected"] == 255).all()
    assert (r["status"] == -1).all() and (r["f_avg"].view(np.uint64) == 2 ** 64 - 1).all() and (r["f_max"].view(np.uint64) == 2 ** 64 - 1).all()


def test_what_the_host_sees_is_refused_and_nothing_is_launched():
    rng = np.random.default_rng(80)
    good = _mixed_videos()[:1] + _mixed_videos()[3:4]
    r = _select_call(good, 0, ws_short=1)
    _untouched(r); assert "workspace" in r["error"]
    for arg in ("descr_dev", "descr", "selected", "f_avg", "f_max", "status", "ws", "summary"):
        r = _select_call(good, 0, null=(arg,))
        _untouched(r); assert "null" in r["error"], arg
    big = dict(means=np.zeros(1025, np.float32), nfps=np.ones(1025, np.int32), n_frames=1025, capacity=153, mask=None)
    r = _select_call([good[0], big], 0)
    _untouched(r); assert "1025 segments" in r["error"]
    r = _select_call(good, 0, override={1: dict(n_segs=0)})
    _untouched(r); assert "0 segments" in r["error"]
    r = _select_call(good, 0, override={0: dict(capacity=(1 << 24) + 1)})
    _untouched(r); assert f"capacity {(1 << 24) + 1}" in r["error"]
    r = _select_call(good, 1, override={0: dict(capacity=-1)})
    _untouched(r); assert "capacity -1" in r["error"]
    crowd = dict(good[0], mask=(rng.random((33, good[0]["n_frames"])) < 0.2).astype(np.uint8))
    r = _select_call([crowd, good[1]], 1)
    _untouched(r); assert "33 annotators" in r["error"]
    for nf in (0, (1 << 24) + 1):
        r = _select_call(good, 0, override={1: dict(n_frames=nf)})
        _untouched(r); assert f"{nf} frames" in r["error"]
    r = _select_call(good, 0, override={1: dict(method=1)})               # one method per call
    _untouched(r); assert "method" in r["error"]
    # offsets outside the outputs: a summary that ends one entry past the buffer, a selection that does, a negative offset
    s_total = 3 + sum(int(v["nfps"].sum()) + 3 for v in good)
    r = _select_call(good, 0, totals=(s_total - 4, 52))
    _untouched(r); assert "outside" in r["error"]
    r = _select_call(good, 0, totals=(s_total, 51))
    _untouched(r); assert "outside" in r["error"]
    r = _select_call(good, 0, override={0: dict(summary0=-1)})
    _untouched(r); assert "outside" in r["error"]
    # and the call goes through with everything in place
    _check(_select_call(good, 0), good, 0.15, 0)


def test_a_device_descriptor_that_disagrees_with_the_host_copy_gets_status_4():
    """The entry point sizes the grids and the workspace by the host copy.  A device copy past it -- 1025 segments, a budget one past the
    call's largest, a video longer than the call's longest, a range outside the outputs -- is given up by the prologue: status 4, NaN
    F-scores, and neither its summary, its selection nor anything else is written."""
    good = _mixed_videos()[:1] + _mixed_videos()[3:5]
    alone = _select_call(good[1:], 0)
    _check(alone, good[1:], 0.15, 0)
    for fields in (dict(n_segs=1025), dict(capacity=9001), dict(capacity=1 << 24), dict(n_users=33), dict(method=2), dict(n_frames=60001),
                   dict(summary0=1 << 40), dict(sel0=-1), dict(n_segs=0)):
        r = _select_call(good, 0, gap=5, dev_override={0: fields})
        assert r["rc"] == 0, r["error"]
        assert r["status"].tolist() == [4, 0, 0], fields
        assert (r["summaries"][0].view(np.uint32) == 0xFFFFFFFF).all() and (r["selected"][0] == 255).all(), fields
        assert np.isnan(r["f_avg"][0]) and np.isnan(r["f_max"][0])
        assert (r["raw"][r["outside"]].view(np.uint32) == 0xFFFFFFFF).all(), fields
        _same_results(r, alone, [(1, 0), (2, 1)], str(fields))


# ------------------------------------------------------------------------------------------------ 5. segments
SEG_LENS = (0, 1, 7, 8, 9, 127, 128, 129, 136, 1000, 70001)
PICK_COUNTS = (1, 2, 4095, 4096, 4097, 5000)


def _segment_videos():
    """Per pick count two videos of 75 000 frames (and two of 50): (a) ascending picks with duplicates, the first pick past frame 0, no pick
    at n_frames (the sentinel interval), a score per pick; (b) the first pick at 0, the last at n_frames (no sentinel), one score fewer than
    intervals.  Segments: every length of SEG_LENS that fits, back to back from frame 3, then the whole video, then an empty one."""
    rng = np.random.default_rng(81)
    vids = []
    for n_picks in PICK_COUNTS:
        for variant, n_frames in (("a", 75000), ("b", 75000), ("a", 50), ("b", 50)):
            if n_frames == 50 and n_picks > 2:
                continue
            if variant == "a":
                picks = np.sort(rng.integers(5, n_frames, size=n_picks)).astype(np.int32)
                if n_picks >= 4:
                    picks[n_picks // 2] = picks[n_picks // 2 - 1]; picks[3] = picks[2] = picks[1]      # duplicates, a triple among them
                assert picks[0] > 0 and picks[-1] != n_frames
                n_int = n_picks
                n_steps = n_picks
            else:
                if n_picks == 1:
                    picks = np.array([0], np.int32)
                else:
                    picks = np.concatenate([[0], np.sort(rng.integers(0, n_frames + 1, size=n_picks - 2)), [n_frames]]).astype(np.int32)
                n_int = n_picks if n_picks == 1 else n_picks - 1
                n_steps = max(n_int - 1, 1)
            cps, at = [], 3
            for L in SEG_LENS:
                if at + L <= n_frames:
                    cps.append((at, at + L - 1)); at += L
            cps += [(0, n_frames - 1), (n_frames, n_frames - 1)]
            vids.append(dict(picks=picks, n_frames=n_frames, n_int=n_int, scores=rng.random(n_steps).astype(np.float32),
                             cps=np.array(cps, np.int32), name=f"{n_picks}{variant}{n_frames}"))
    assert any(v["cps"].shape[0] == len(SEG_LENS) + 2 for v in vids)
    return vids


def _segments_call(vids, entry="long", override=None, dev_override=None, gap=7):
    from summarizer_amd import _lib
    lib, dev, n = _lib.load(), _dev(), len(vids)
    scores = torch.from_numpy(np.concatenate([v["scores"] for v in vids])).to(dev)
    picks = [torch.from_numpy(v["picks"]).to(dev) for v in vids]
    cps = [torch.from_numpy(np.ascontiguousarray(v["cps"])).to(dev) for v in vids]
    descr = (_lib.EvalDevVideo * n)()
    row0, frame0, seg0, franges, sranges = 0, gap, gap, [], []
    for i, v in enumerate(vids):
        e = descr[i]
        e.picks, e.n_picks, e.n_frames, e.n_steps, e.row0, e.frame0 = picks[i].data_ptr(), len(v["picks"]), v["n_frames"], len(v["scores"]), row0, frame0
        e.cps, e.n_segs, e.seg0 = cps[i].data_ptr(), v["cps"].shape[0], seg0
        franges.append((frame0, frame0 + v["n_frames"])); sranges.append((seg0, seg0 + v["cps"].shape[0]))
        row0 += len(v["scores"]); frame0 += v["n_frames"] + gap; seg0 += v["cps"].shape[0] + gap
        for k, val in (override or {}).get(i, {}).items():
            setattr(e, k, val)
    on_dev = (_lib.EvalDevVideo * n).from_buffer_copy(bytes(descr))
    for i, fields in (dev_override or {}).items():
        for k, val in fields.items():
            setattr(on_dev[i], k, val)
    descr_dev = torch.frombuffer(bytearray(bytes(on_dev)), dtype=torch.uint8).to(dev)
    scratch, seg = _poisoned(frame0, torch.float32, dev), _poisoned(seg0, torch.float32, dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if entry == "long":
        rc = lib.sumk_eval_device_segments_long(scores.data_ptr(), descr_dev.data_ptr(), C.cast(descr, C.c_void_p), n, scratch.data_ptr(), seg.data_ptr(), st)
    else:
        rc = lib.sumk_eval_device_segments(scores.data_ptr(), descr_dev.data_ptr(), n, scratch.data_ptr(), seg.data_ptr(), st)
    torch.cuda.synchronize(dev)
    fr, sg = scratch.cpu().numpy(), seg.cpu().numpy()
    f_out, s_out = np.ones(fr.shape[0], bool), np.ones(sg.shape[0], bool)
    for lo, hi in franges:
        f_out[lo:hi] = False
    for lo, hi in sranges:
        s_out[lo:hi] = False
    return dict(rc=rc, frames=[fr[lo:hi] for lo, hi in franges], means=[sg[lo:hi] for lo, hi in sranges], raw_frames=fr, raw_means=sg,
                frames_outside=f_out, means_outside=s_out, error=lib.sumk_last_error().decode(errors="replace"))


def _leaf_sum(a):
    """np_pairwise_leaf of csrc/evaldev_common.h in float32 numpy operations (n <= 128)."""
    n = a.shape[0]
    if n < 8:
        r = np.float32(0)
        for x in a:
            r = np.float32(r + x)
        return r
    r = a[:8].copy()
    for i in range(8, n - n % 8, 8):
        r = r + a[i:i + 8]
    res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3])) + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
    for x in a[n - n % 8:]:
        res = np.float32(res + x)
    return res


def _tree_sum(a):
    """np_pairwise_tree of csrc/evaldev_common.h: numpy's pairwise tree over the whole of `a`."""
    n = a.shape[0]
    if n <= 128:
        return _leaf_sum(a)
    n2 = n // 2
    n2 -= n2 % 8
    return np.float32(_tree_sum(a[:n2]) + _tree_sum(a[n2:]))


def _np_sum(a):
    """np_pairwise_sum of csrc/evaldev_common.h: the tree per block of 8192 values (numpy's buffer size), the blocks added in order."""
    r = _tree_sum(a[:8192])
    for i in range(8192, a.shape[0], 8192):
        r = np.float32(r + _tree_sum(a[i:i + 8192]))
    return r


def test_segments_equal_numpy_the_block_sums_and_the_block_kernel():
    """Against `frame_scores[lo:hi + 1].mean()` itself, against the additions written out (`_np_sum`: past 8192 frames a segment is several
    of numpy's buffer blocks) and against sumk_eval_device_segments wherever it takes the video -- every segment length of SEG_LENS, the
    whole video of 75 000 frames and an empty segment on every video."""
    from summarizer_amd.utils import eval as E
    vids = _segment_videos()
    got = _segments_call(vids)
    assert got["rc"] == 0, got["error"]
    long_ = 0
    for i, v in enumerate(vids):
        frames = E.upsample(v["scores"], v["n_frames"], v["picks"])
        assert frames.dtype == np.float32
        np.testing.assert_array_equal(got["frames"][i], frames, err_msg=v["name"])
        want = np.array([frames[lo:hi + 1].mean() if hi >= lo else np.float32(0) for lo, hi in v["cps"]], np.float32)
        np.testing.assert_array_equal(got["means"][i], want, err_msg=v["name"])
        written = np.array([_np_sum(frames[lo:hi + 1]) / np.float32(hi + 1 - lo) if hi >= lo else np.float32(0) for lo, hi in v["cps"]], np.float32)
        np.testing.assert_array_equal(got["means"][i], written, err_msg=v["name"])
        long_ += sum(hi + 1 - lo > 8192 for lo, hi in v["cps"])
    assert long_ == 24                                                                          # 70 001 frames and the whole video, 12 videos
    assert (got["raw_frames"][got["frames_outside"]].view(np.uint32) == 0xFFFFFFFF).all()
    assert (got["raw_means"][got["means_outside"]].view(np.uint32) == 0xFFFFFFFF).all()
    old = [i for i, v in enumerate(vids) if v["n_int"] <= OLD_MAX_INT]
    assert {len(vids[i]["picks"]) for i in old} == {1, 2, 4095, 4096, 4097}                   # (4097 picks with the last at n_frames: 4096 intervals)
    assert any(vids[i]["n_frames"] == 75000 for i in old)                                       # (the long segments are among them)
    block = _segments_call([vids[i] for i in old], entry="block")
    assert block["rc"] == 0, block["error"]
    for k, i in enumerate(old):
        np.testing.assert_array_equal(got["frames"][i], block["frames"][k], err_msg=vids[i]["name"])
        np.testing.assert_array_equal(got["means"][i], block["means"][k], err_msg=vids[i]["name"])


def test_segments_refusals_launch_nothing_and_a_bad_device_copy_stays_inside():
    vids = _segment_videos()[:3]
    for fields, word in ((dict(n_picks=0), "0 picks"), (dict(n_picks=(1 << 20) + 1), "picks"), (dict(n_frames=0), "0 frames"),
                         (dict(n_frames=(1 << 24) + 1), "frames"), (dict(n_segs=-1), "segments")):
        r = _segments_call(vids, override={1: fields})
        assert r["rc"] == -1 and word in r["error"], (fields, r["error"])
        assert (r["raw_frames"].view(np.uint32) == 0xFFFFFFFF).all() and (r["raw_means"].view(np.uint32) == 0xFFFFFFFF).all()
    good = _segments_call(vids)
    assert good["rc"] == 0
    # a device copy past the limits: NaN segment means for that video, no frame written, the others untouched
    r = _segments_call(vids, dev_override={1: dict(n_picks=(1 << 20) + 1)})
    assert r["rc"] == 0 and np.isnan(r["means"][1]).all() and (r["frames"][1].view(np.uint32) == 0xFFFFFFFF).all()
    for i in (0, 2):
        np.testing.assert_array_equal(r["frames"][i], good["frames"][i]); np.testing.assert_array_equal(r["means"][i], good["means"][i])
    assert (r["raw_frames"][r["frames_outside"]].view(np.uint32) == 0xFFFFFFFF).all()
    assert (r["raw_means"][r["means_outside"]].view(np.uint32) == 0xFFFFFFFF).all()
    # change points outside the video on the device copy are clamped, as in the one-workgroup kernel
    wild = [dict(v) for v in vids]
    wild[0] = dict(wild[0], cps=np.array([(-5, 10), (70, 10 ** 6), (2 * 10 ** 6, 3 * 10 ** 6)], np.int32))
    a, b = _segments_call(wild), _segments_call(wild, entry="block")
    assert a["rc"] == 0 and b["rc"] == 0
    np.testing.assert_array_equal(a["means"][0], b["means"][0])


# ------------------------------------------------------------------------------------------------ 6. Summarizer(device=True, tail="long")
@pytest.fixture(scope="module")
def long_inputs():
    from summarizer_amd.models.logistic import LogisticRegression
    dev = _dev()
    torch.manual_seed(6)
    model = LogisticRegression(input_size=64).eval().to(dev)
    rng = np.random.default_rng(82)
    feats = []
    for T, seed in ((4100, 1), (300, 2)):
        # piecewise-stationary features: change points worth finding, scores that differ between segments
        bounds = np.sort(rng.choice(np.arange(1, T), size=12, replace=False))
        level = np.repeat(rng.standard_normal((13, 64)).astype(np.float32), np.diff(np.concatenate([[0], bounds, [T]])), axis=0)
        feats.append(torch.from_numpy(level + 0.1 * rng.standard_normal((T, 64)).astype(np.float32)).to(dev))
    picks = [(15 * np.arange(4100)).astype(np.int32), None]
    return model, feats, picks, [61500, None]


@pytest.mark.parametrize("method", ["knapsack", "rank"])
def test_summarizer_long_tail_equals_the_host(method, long_inputs):
    import summarizer_amd
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    model, feats, picks, n_frames = long_inputs
    opts = dict(proportion=0.15, method=method, kts="banded", max_ncp=40, lmax=512)
    assert eval_native.select_capacity(61500, 0.15) == 9225 > OLD_MAX_CAP and feats[0].shape[0] > 4096
    with pytest.raises(_lib.SumkError, match="4100 picks"):                                   # the default tail refuses the video
        summarizer_amd.Summarizer(model, device=True, **opts).summarize(feats[0], picks[0], n_frames[0])
    for sub in ([0], [0, 1]):
        f, p, nf = [feats[i] for i in sub], [picks[i] for i in sub], [n_frames[i] for i in sub]
        host = summarizer_amd.Summarizer(model, device=False, **opts).summarize_batch(f, p, nf)
        ondev = summarizer_amd.Summarizer(model, device=True, tail="long", **opts).summarize_batch(f, p, nf)
        assert len(host) == len(ondev) == len(sub)
        for h, d in zip(host, ondev):
            assert all(torch.is_tensor(d[k]) and d[k].is_cuda for k in ("scores", "machine_summary", "change_points", "n_frame_per_seg", "n_segs", "status"))
            S = int(d["n_segs"])
            assert S == h["change_points"].shape[0] and int(d["status"]) == 0 and d["change_points"].shape[0] == 41
            np.testing.assert_array_equal(d["scores"].cpu().numpy(), h["scores"])
            np.testing.assert_array_equal(d["change_points"].cpu().numpy()[:S], h["change_points"])
            np.testing.assert_array_equal(d["n_frame_per_seg"].cpu().numpy()[:S], h["n_frame_per_seg"])
            assert (d["n_frame_per_seg"].cpu().numpy()[S:] == 0).all()
            np.testing.assert_array_equal(d["machine_summary"].cpu().numpy(), h["machine_summary"])
            assert d["machine_summary"].dtype == torch.float32
        assert host[0]["change_points"].shape[0] > 5 and 0 < host[0]["machine_summary"].sum() <= 9225
    # a short video alone: the long tail gives what the default tail gives
    block = summarizer_amd.Summarizer(model, device=True, **opts).summarize(feats[1])
    long_ = summarizer_amd.Summarizer(model, device=True, tail="long", **opts).summarize(feats[1])
    for k in ("scores", "machine_summary", "change_points", "n_frame_per_seg", "n_segs", "status"):
        np.testing.assert_array_equal(long_[k].cpu().numpy(), block[k].cpu().numpy(), err_msg=k)


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_long_segments_and_select_replay_from_a_graph():
    """Every launch of the chain ends by itself and its count is host-known: the two calls on fixed buffers capture into one linear graph
    (2 + 4 + n_segs launches) and replay with new scores (the test of tests/test_gpu_select.py, with the long entries)."""
    import recipes as R
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    lib, dev = _lib.load(), _dev()
    rng = np.random.default_rng(83)
    raw = [R.synthetic_video(T, 8700 + i, n_users=U) for i, (T, U) in enumerate([(120, 3), (45, 1), (200, 7)])]
    vids = [eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"], E.rank_users(v["user_scores"]))
            for v in raw]
    lens, n = [120, 45, 200], 3
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
    ws = _poisoned(lib.sumk_eval_device_select_long_workspace_bytes(n, max(q.n_segs for q in sd), max(q.capacity for q in sd)), torch.uint8, dev)

    def enqueue():
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.sumk_eval_device_segments_long(scores.data_ptr(), vd_dev.data_ptr(), C.cast(vd, C.c_void_p), n, scratch.data_ptr(), seg.data_ptr(), st),
                   "segments_long")
        _lib.check(lib.sumk_eval_device_select_long(sd_dev.data_ptr(), C.cast(sd, C.c_void_p), n, summary.data_ptr(), total, selected.data_ptr(), segs,
                                                    f.data_ptr(), f.data_ptr() + 8 * n, status.data_ptr(), ws.data_ptr(), ws.numel(), st), "select_long")
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                    # one capture stream, the launches in order: a linear graph
        enqueue()
    for rep in range(2):
        s = [rng.random(T).astype(np.float32) for T in lens]
        scores.copy_(torch.from_numpy(np.concatenate(s)).to(dev))
        for t in (summary, selected, f, status, ws, seg, scratch):
            t.view(torch.uint8).fill_(255)
        g.replay()
        torch.cuda.synchronize(dev)
        want = eval_native.evaluate_batch(vids, s, 0.15, "knapsack", want_summaries=True, n_threads=2)
        assert status.cpu().tolist() == [0, 0, 0]
        np.testing.assert_array_equal(f.cpu().numpy()[:n], want[1]); np.testing.assert_array_equal(f.cpu().numpy()[n:], want[2])
        np.testing.assert_array_equal(summary.cpu().numpy(), np.concatenate(want[3]))
