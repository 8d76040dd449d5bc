"""Batch evaluation tail in native threads (libsumk.so: `sumk_eval_videos`, csrc/evaltail.hip): for a list of videos it
does what `utils/eval.py` does one video at a time in numpy -- upsample, key-shot summary (knapsack / rank), F-scores
against the annotators and the rank correlation -- with bit-identical summaries and F-scores (tests/test_host_eval.py)
and the correlation equal to ~1e-15.  Both metrics of `evaluate_scores` run here: `metric="spearmanr"` (the default) and
`metric="kendalltau"` (tau-b from integer pair counts in O(n log n): `sumk_eval_videos_kendall` in the host threads,
`sumk_eval_device_kendall` -- csrc/evalkendall.hip -- with the scores still in HBM; tests/test_host_kendall.py,
tests/test_gpu_kendall.py).  This is what `Trainer.test` / `predict_dataset` call; the numpy functions stay the readable
specification."""
import ctypes as C
import math
import numpy as np

from .. import _lib

METHODS = {"knapsack": 0, "rank": 1}
METRICS = ("spearmanr", "kendalltau")
KENDALL_MAX_FRAMES = 16384      # KD_MAX_FRAMES of csrc/evaldev_common.h: frames per video the device Kendall kernel sorts in LDS
# limits of sumk_eval_device_select (include/sumk.h SUMK_SELECT_*; csrc/evalselect.hip): segments, frame budget and annotators per video
SELECT_MAX_SEGS, SELECT_MAX_CAPACITY, SELECT_MAX_USERS, SELECT_MAX_FRAMES = 1024, 8191, 32, 1 << 24
SELECT_LDS_CAPACITY = 4095      # the knapsack's profit rows stay in LDS up to this budget and move to the workspace above it
SELECTS = ("host", "device")
# limits of the long-video tail (include/sumk.h SUMK_SEGMENTS_LONG_* / SUMK_SELECT_LONG_*; csrc/evallong.hip): picks and frames per video of
# sumk_eval_device_segments_long; frame budget, capacities per DP block and frame chunks per video of sumk_eval_device_select_long
SEGMENTS_LONG_MAX_PICKS, SEGMENTS_LONG_MAX_FRAMES = 1 << 20, 1 << 24
SELECT_LONG_MAX_CAPACITY, SELECT_LONG_CHUNK, SELECT_LONG_FRAME_CHUNKS = 1 << 24, 2048, 64
# the long-video rank correlation (include/sumk.h SUMK_CORR_LONG_TILE; csrc/evalcorr_long.hip): keys a workgroup sorts in LDS, sorted groups
# per scan block, frames per Spearman chunk and chunks per video at most, bytes of a video's header in the workspace
CORR_LONG_TILE, CORR_LONG_SCAN_BLOCK, CORR_LONG_CHUNK_FRAMES, CORR_LONG_MAX_CHUNKS, CORR_LONG_HEADER_BYTES = 2048, 1024, 4096, 256, 72
CORR_LONG_MAX_USERS = 32
TAILS = ("block", "long")


def _check_metric(metric):
    if metric not in METRICS:
        raise KeyError(f"Unknown metric {metric}")


def _split_counts(flat, users):
    """(sum(users), 4) int64 {cmd, xtie, ytie, ntie} rows -> one (n_users, 4) array per video."""
    return [a.copy() for a in np.split(flat.reshape(-1, 4), np.cumsum(users)[:-1])] if users else []


def prepare_video(n_frames, picks, cps=None, nfps=None, user_summary=None, user_ranks=None):
    """Contiguous, C-typed copies of one video's constant evaluation metadata (done once per video, then cached)."""
    picks = np.asarray(picks)
    if picks.dtype != int:                                   # eval.py:25-26
        picks = picks.astype(np.int32)
    d = dict(n_frames=int(n_frames), picks=np.ascontiguousarray(picks, dtype=np.int32))
    if cps is not None:
        d["cps"] = np.ascontiguousarray(np.asarray(cps)[:, :2], dtype=np.int32)
        d["nfps"] = np.ascontiguousarray(np.asarray(nfps), dtype=np.int32)
    if user_summary is not None:
        d["user_summary"] = np.ascontiguousarray(user_summary, dtype=np.float32)
    if user_ranks is not None:
        d["user_ranks"] = np.ascontiguousarray(user_ranks, dtype=np.float64)
    return d


def evaluate_batch(videos, scores, proportion=0.15, method="knapsack", want_summaries=False, n_threads=0, metric="spearmanr", counts_out=None):
    """videos: list of `prepare_video` dicts; scores: list of (n_steps,) float32 arrays.
    Returns (corr (n,), f_avg (n,), f_max (n,), summaries or None); entries are NaN where the inputs were not given.
    metric: "spearmanr" | "kendalltau" (tau-b), as `eval.evaluate_scores`.  counts_out (Kendall only): a list that receives, per video, the
    (n_users, 4) int64 pair counts {cmd, xtie, ytie, ntie} the values were computed from."""
    if method not in METHODS:
        raise KeyError(f"Unknown method {method}")
    _check_metric(metric)
    kendall = metric == "kendalltau"
    lib = _lib.load()
    n = len(videos)
    arr = (_lib.EvalVideo * max(n, 1))()
    keep, summaries = [], []
    for i, (v, s) in enumerate(zip(videos, scores)):
        s = np.ascontiguousarray(np.atleast_1d(s), dtype=np.float32)
        keep.append(s)
        e = arr[i]
        e.scores, e.n_steps = s.ctypes.data, s.shape[0]
        e.picks, e.n_picks, e.n_frames = v["picks"].ctypes.data, v["picks"].shape[0], v["n_frames"]
        if "cps" in v:
            e.cps, e.nfps, e.n_segs = v["cps"].ctypes.data, v["nfps"].ctypes.data, v["cps"].shape[0]
            if want_summaries:
                out = np.empty(int(v["nfps"].sum()), dtype=np.float32)
                summaries.append(out)
                e.machine_summary = out.ctypes.data
        if "user_summary" in v and "cps" in v:
            if v["user_summary"].shape[1] != v["n_frames"]:
                raise ValueError(f"user_summary has {v['user_summary'].shape[1]} frames, video has {v['n_frames']}")
            e.user_summary, e.n_users = v["user_summary"].ctypes.data, v["user_summary"].shape[0]
        if "user_ranks" in v:
            if not kendall:                   # (Kendall: handed over after sumk_eval_videos, which then leaves Spearman out)
                e.user_ranks = v["user_ranks"].ctypes.data
            e.n_users = v["user_ranks"].shape[0] if e.n_users == 0 else e.n_users
    _lib.check(lib.sumk_eval_videos(C.cast(arr, C.c_void_p), n, float(proportion), METHODS[method], int(n_threads)),
               "sumk_eval_videos")
    if kendall:
        users = [v["user_ranks"].shape[0] if "user_ranks" in v else 0 for v in videos]
        for e, v in zip(arr, videos):
            if "user_ranks" in v:
                if v["user_ranks"].shape[0] != e.n_users or v["user_ranks"].shape[1] != v["n_frames"]:
                    raise ValueError(f"user_ranks is {v['user_ranks'].shape}, video has {e.n_users} annotators and {v['n_frames']} frames")
                e.user_ranks = v["user_ranks"].ctypes.data
        counts = np.zeros(4 * max(sum(users), 1), dtype=np.int64) if counts_out is not None else None
        _lib.check(lib.sumk_eval_videos_kendall(C.cast(arr, C.c_void_p), n, counts.ctypes.data if counts is not None else None, int(n_threads)),
                   "sumk_eval_videos_kendall")
        if counts_out is not None:
            counts_out[:] = _split_counts(counts[:4 * sum(users)], users)
    corr = np.array([arr[i].corr for i in range(n)]); f_avg = np.array([arr[i].f_avg for i in range(n)])
    f_max = np.array([arr[i].f_max for i in range(n)])
    return corr, f_avg, f_max, (summaries if want_summaries else None)


# ---------------------------------------------------------------------------------------------- device-side part (csrc/evaldev.hip)
def device_ready(v):
    """Can this video's tail run on the device?  (ascending picks, <= 4096 of them, <= 32 annotators, change points + ranks present)
    A property of the video's constant metadata: computed once and kept in the prepare_video dict (Trainer.test asks for every video
    of a fold on every call -- 0.5 ms of numpy per 50 videos when recomputed)."""
    r = v.get("_dev_ready")
    if r is None:
        p = v["picks"]
        r = v["_dev_ready"] = bool("cps" in v and "user_ranks" in v and 0 < p.shape[0] <= 4096 and v["user_ranks"].shape[0] <= 32
                                   and bool(np.all(np.diff(p) >= 0)) and v["user_ranks"].shape[1] == v["n_frames"])
    return r


class SelectStatusError(_lib.SumkError):
    """evaluate_batch_device(select="device"): sumk_eval_device_select gave a video up for something only the device sees (a nonzero
    status: a non-finite or huge segment mean, segment values past the int32 profit rows).  The host tail takes such a batch."""


def select_capacity(n_frames, proportion):
    """The frame budget of a summary, as eval_one takes it: floor((double)n_frames * proportion)."""
    return int(math.floor(float(int(n_frames)) * float(proportion)))


def select_refusal(n_segs, n_frames, n_users, proportion):
    """None when a video of this geometry is within the limits of sumk_eval_device_select, else the limit it is past, in words."""
    cap = select_capacity(n_frames, proportion)
    if not 1 <= n_segs <= SELECT_MAX_SEGS:
        return f"{n_segs} segments (1 .. {SELECT_MAX_SEGS})"
    if not 0 <= cap <= SELECT_MAX_CAPACITY:
        return f"a budget of {cap} frames = floor({n_frames} x {proportion}) (0 .. {SELECT_MAX_CAPACITY})"
    if not 0 <= n_users <= SELECT_MAX_USERS:
        return f"{n_users} annotators (at most {SELECT_MAX_USERS})"
    if not 1 <= n_frames <= SELECT_MAX_FRAMES:
        return f"{n_frames} frames (1 .. {SELECT_MAX_FRAMES})"
    return None


def select_long_refusal(n_segs, n_frames, n_users, proportion):
    """select_refusal for sumk_eval_device_select_long: the same limits but for the frame budget, which may reach SELECT_LONG_MAX_CAPACITY."""
    cap = select_capacity(n_frames, proportion)
    if not 1 <= n_segs <= SELECT_MAX_SEGS:
        return f"{n_segs} segments (1 .. {SELECT_MAX_SEGS})"
    if not 0 <= cap <= SELECT_LONG_MAX_CAPACITY:
        return f"a budget of {cap} frames = floor({n_frames} x {proportion}) (0 .. {SELECT_LONG_MAX_CAPACITY})"
    if not 0 <= n_users <= SELECT_MAX_USERS:
        return f"{n_users} annotators (at most {SELECT_MAX_USERS})"
    if not 1 <= n_frames <= SELECT_MAX_FRAMES:
        return f"{n_frames} frames (1 .. {SELECT_MAX_FRAMES})"
    return None


def select_long_workspace_bytes(n_videos, max_n_segs, max_capacity):
    """The formula of sumk_eval_device_select_long_workspace_bytes (include/sumk.h), for a caller that wants the size before it loads the
    library's answer: per video, each part rounded up to 256 bytes, the improvement bits, two int32 profit rows, the item tables and the
    partial counts of the frame chunks.  The bits are what grows: n_segs x capacity / 8 bytes."""
    def up(b):
        return (b + 255) // 256 * 256
    bits = up(max_n_segs * ((max_capacity + 1 + 63) // 64) * 8)
    rows = up(2 * (max_capacity + 1) * 4)
    items = up((5 * max_n_segs + 9) * 4)
    counts = up(SELECT_LONG_FRAME_CHUNKS * (2 * SELECT_MAX_USERS + 1) * 4)
    return n_videos * (bits + rows + items + counts)


def corr_long_refusal(n_picks, n_frames, n_users):
    """None when a video of this geometry is within the limits of sumk_eval_device_spearman_long / sumk_eval_device_kendall_long, else the
    limit it is past, in words."""
    if not 1 <= n_picks <= SEGMENTS_LONG_MAX_PICKS:
        return f"{n_picks} picks (1 .. {SEGMENTS_LONG_MAX_PICKS})"
    if not 1 <= n_frames <= SEGMENTS_LONG_MAX_FRAMES:
        return f"{n_frames} frames (1 .. {SEGMENTS_LONG_MAX_FRAMES})"
    if n_users > CORR_LONG_MAX_USERS:
        return f"{n_users} annotators (at most {CORR_LONG_MAX_USERS})"
    return None


def corr_long_workspace_bytes(geometries, metric="spearmanr"):
    """The formula of sumk_eval_device_spearman_long_workspace_bytes / sumk_eval_device_kendall_long_workspace_bytes (include/sumk.h) for
    videos of (n_picks, n_frames, n_users): each part rounded up to 256 bytes -- the headers, two buffers of group keys, two prefix sums and
    the scan blocks; Spearman: the groups' ranks and 33 partial sums per chunk of frames; Kendall: the dense x ranks, two buffers of 64-bit
    frame keys (16 bytes per annotator and frame) and the integer counters.  0 for a geometry past a limit, as the library answers."""
    _check_metric(metric)
    geometries = list(geometries)
    if not 1 <= len(geometries) <= 65535 or any(corr_long_refusal(*g) is not None for g in geometries):
        return 0

    def up(b):
        return (b + 255) // 256 * 256
    G = sum(p + 1 for p, _, _ in geometries)
    B = sum((p + 1 + CORR_LONG_SCAN_BLOCK - 1) // CORR_LONG_SCAN_BLOCK for p, _, _ in geometries)
    U = sum(max(u, 0) for _, _, u in geometries)
    total = up(CORR_LONG_HEADER_BYTES * len(geometries)) + 2 * up(8 * G) + 2 * up(4 * G) + up(8 * B)
    if metric == "kendalltau":
        UF = sum(max(u, 0) * f for _, f, u in geometries)
        return total + up(4 * G) + 2 * up(8 * UF) + up(8 * (2 * U + len(geometries)))
    chunks = sum(min(CORR_LONG_MAX_CHUNKS, max(1, (f + CORR_LONG_CHUNK_FRAMES - 1) // CORR_LONG_CHUNK_FRAMES)) for _, f, _ in geometries)
    return total + up(8 * G) + up(8 * (CORR_LONG_MAX_USERS + 1) * chunks)


def select_device_ready(v, proportion=0.15):
    """Can this video's key-shot selection, summary and F-scores run on the device (sumk_eval_device_select)?  The one mirror of that
    call's limits: change points present, <= 1024 segments of non-negative length, floor(n_frames * proportion) <= 8191, <= 32
    annotators whose summaries span n_frames."""
    if "cps" not in v:
        return False
    nfps, us = v["nfps"], v.get("user_summary")
    if nfps.shape[0] != v["cps"].shape[0] or (nfps.shape[0] and (int(nfps.min()) < 0 or int(nfps.sum(dtype=np.int64)) >= 2 ** 31)):
        return False
    if us is not None and us.shape[1] != v["n_frames"]:
        return False
    return select_refusal(v["cps"].shape[0], v["n_frames"], 0 if us is None else us.shape[0], proportion) is None


_DEV_BATCH_CACHE = {}      # (ids of the videos' dicts, lens, device) -> the batch's constant descriptors (device + host side); a few entries


def kendall_device_ready(v):
    """device_ready, and few enough frames for the Kendall kernel's LDS-resident sort (longer videos take the native host path)."""
    return device_ready(v) and v["n_frames"] <= KENDALL_MAX_FRAMES


def device_ready_long(v):
    """Can this video's tail run on the device with tail="long" (sumk_eval_device_segments_long and the long rank correlation)?  device_ready
    with the limits of those calls: ascending picks, 1 .. 1 048 576 of them, 1 .. 2^24 frames, <= 32 annotators, change points and ranks
    present.  The frame count does not depend on the metric: kendall_device_ready is not consulted."""
    r = v.get("_dev_ready_long")
    if r is None:
        p = v["picks"]
        r = v["_dev_ready_long"] = bool("cps" in v and "user_ranks" in v and v["user_ranks"].shape[1] == v["n_frames"]
                                        and corr_long_refusal(p.shape[0], v["n_frames"], v["user_ranks"].shape[0]) is None
                                        and bool(np.all(np.diff(p) >= 0)))
    return r


def _kendall_meta(v):
    """Annotator side of Kendall's tau, constants of the video: dense ranks int32 (n_users, n_frames), ascending with the annotator's
    score, and tied pairs int64 (n_users,)."""
    m = v.get("_kendall")
    if m is None:
        ru = v["user_ranks"]
        dense = np.empty(ru.shape, dtype=np.int32)
        ytie = np.zeros(ru.shape[0], dtype=np.int64)
        for u in range(ru.shape[0]):
            _, inv, cnt = np.unique(-ru[u], return_inverse=True, return_counts=True)      # (user_ranks descend with the score: rankdata(-y))
            dense[u] = inv.reshape(-1)
            cnt = cnt.astype(np.int64)
            ytie[u] = int((cnt * (cnt - 1) // 2).sum())
        m = v["_kendall"] = (dense, ytie)
    return m


def _device_meta(v, device, kendall=False, select=False):
    """The video's constant metadata as device tensors, uploaded once and cached inside the prepare_video dict
    (kendall: with the annotators' dense ranks and tie counts, which only the Kendall launch reads; select: with the frames per segment
    and the annotators' summaries binarised to uint8, which only the select launch reads)."""
    import torch
    cache = v.setdefault("_dev", {})
    d = cache.get(str(device))
    if select:
        d = _device_meta(v, device) if d is None else d
        if "nfps" not in d:
            d["nfps"] = torch.from_numpy(v["nfps"]).to(device)
            d["mask"] = torch.from_numpy((v["user_summary"] > 0).astype(np.uint8)).to(device) if "user_summary" in v else None
        return d
    if kendall and d is not None and "ydense" not in d:
        dense, ytie = _kendall_meta(v)
        d["ydense"], d["ytie"] = torch.from_numpy(dense).to(device), torch.from_numpy(ytie).to(device)
    if d is None:
        ru = v["user_ranks"]
        mu = ru.sum(axis=1) / ru.shape[1]
        d = cache[str(device)] = dict(
            picks=torch.from_numpy(v["picks"]).to(device), cps=torch.from_numpy(v["cps"]).to(device),
            ranks=torch.from_numpy(ru).to(device), mean=torch.from_numpy(mu).to(device),
            ssq=torch.from_numpy(((ru - mu[:, None]) ** 2).sum(axis=1)).to(device))
        if kendall:
            return _device_meta(v, device, True)
    return d


def evaluate_batch_device(videos, scores_dev, lens, proportion=0.15, method="knapsack", want_summaries=False, n_threads=0, metric="spearmanr",
                          counts_out=None, select="host", tail="block", max_workspace_bytes=None):
    """The same evaluation with the scores still in HBM: `scores_dev` = packed (sum(lens),) float32 device tensor, video i owning rows
    [sum(lens[:i]), sum(lens[:i + 1])).  One launch (a block per video) does upsample + float32 segment means + Spearman on the device
    (sumk_eval_device); one small D2H brings the segment means and correlations home; key-shot selection, summary expansion and
    F-scores finish in the native host threads (sumk_eval_videos with seg_means given).  Same return value as evaluate_batch.
    metric="kendalltau": sumk_eval_device_kendall (a workgroup per video and annotator) takes the Spearman launch's place; every video
    must then pass kendall_device_ready.  counts_out: as in evaluate_batch.
    select="device": the selection, the summaries and the F-scores stay on the device too (sumk_eval_device_select, enqueued between the
    segments kernel and the correlation); ONE D2H at the end carries corr, f_avg, f_max and the per-video status (plus the summaries
    when asked for), no host thread runs.  Every video must pass select_device_ready(v, proportion); a nonzero status raises
    SelectStatusError (a SumkError), after which select="host" on the same batch is the way to its numbers.
    tail="long": the same call for videos past the one-workgroup limits (4096 picks; Kendall: 16 384 frames; select="device": a budget of
    8191 frames) -- sumk_eval_device_segments_long, sumk_eval_device_spearman_long / sumk_eval_device_kendall_long and (select="device")
    sumk_eval_device_select_long take the places of the block kernels.  Every video must pass device_ready_long(v); the workspaces of the
    correlation and the selection are checked against max_workspace_bytes (None: utils.kts.DEFAULT_MAX_WORKSPACE_BYTES) before anything
    is enqueued, a refusal raises SumkError with the bytes needed.  Same results: summaries, F-scores and Kendall bit for bit, Spearman to
    float64 re-association.  tail="block" (the default) ignores max_workspace_bytes."""
    import torch
    if method not in METHODS:
        raise KeyError(f"Unknown method {method}")
    if select not in SELECTS:
        raise KeyError(f"Unknown select {select}")
    if tail not in TAILS:
        raise KeyError(f"Unknown tail {tail}")
    _check_metric(metric)
    kendall = metric == "kendalltau"
    lib = _lib.load()
    n, dev = len(videos), scores_dev.device
    if n == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0), ([] if want_summaries else None)
    if not scores_dev.is_cuda or scores_dev.dtype != torch.float32 or not scores_dev.is_contiguous():
        raise _lib.SumkError("evaluate_batch_device: scores must be a contiguous float32 GPU tensor")
    if tail == "long":
        return _evaluate_long(lib, videos, scores_dev, lens, proportion, method, want_summaries, n_threads, kendall, counts_out, select, max_workspace_bytes)
    # Everything below that depends only on WHICH videos are scored at WHICH lengths -- the validity checks, the device descriptor block and
    # the constant fields of the host descriptors -- is built once per (videos, lens, device) and kept: a fold's test set is the same on
    # every Trainer.test call.
    key = (tuple(id(v) for v in videos), tuple(int(T) for T in lens), str(dev))
    ent = _DEV_BATCH_CACHE.get(key)
    if ent is None:
        # the kernel's fixed-size LDS tables and its rank rule: the same conditions Trainer._test_on_device tests before coming here
        # (a direct caller past them would corrupt LDS silently: the descriptors live in device memory, sumk_eval_device cannot look)
        for i, (v, T) in enumerate(zip(videos, lens)):
            if not device_ready(v):
                raise _lib.SumkError(f"evaluate_batch_device: video {i} does not qualify for the device tail (needs ascending picks, <= 4096 of "
                                     "them, <= 32 annotators, change points and annotator ranks over n_frames); use evaluate_batch")
            # eval.py:26-34 (upsample): intervals = picks + the n_frames sentinel; one interval per score -- the host tail returns an error
            # for more intervals than scores (csrc/evaltail.hip eval_one), where the reference's loop raises IndexError
            n_picks = v["picks"].shape[0]
            n_int = n_picks - 1 + (1 if v["picks"][-1] != v["n_frames"] else 0)
            if n_int > int(T) + 1:
                raise _lib.SumkError(f"evaluate_batch_device: video {i} has {n_int} pick intervals for {int(T)} scores")
        descr = (_lib.EvalDevVideo * n)()
        metas, row0, frame0, seg0 = [], 0, 0, 0
        for i, (v, T) in enumerate(zip(videos, lens)):
            m = _device_meta(v, dev); metas.append(m)
            e = descr[i]
            e.picks, e.n_picks, e.n_frames, e.n_steps = m["picks"].data_ptr(), v["picks"].shape[0], v["n_frames"], int(T)
            e.row0, e.frame0 = row0, frame0
            e.cps, e.n_segs, e.seg0 = m["cps"].data_ptr(), v["cps"].shape[0], seg0
            e.user_ranks, e.user_mean, e.user_ssq, e.n_users = m["ranks"].data_ptr(), m["mean"].data_ptr(), m["ssq"].data_ptr(), v["user_ranks"].shape[0]
            row0 += int(T); frame0 += v["n_frames"]; seg0 += v["cps"].shape[0]
        descr_dev = torch.frombuffer(bytearray(bytes(descr)), dtype=torch.uint8).to(dev)
        if len(_DEV_BATCH_CACHE) >= 8:
            _DEV_BATCH_CACHE.pop(next(iter(_DEV_BATCH_CACHE)))
        # (the entry holds the video dicts themselves: their ids stay theirs for as long as the entry lives)
        ent = _DEV_BATCH_CACHE[key] = dict(videos=list(videos), metas=metas, descr_dev=descr_dev, rows=row0, frames=frame0, segs=seg0)
    descr_dev, row0, frame0, seg0 = ent["descr_dev"], ent["rows"], ent["frames"], ent["segs"]
    if row0 != scores_dev.numel():
        raise _lib.SumkError(f"evaluate_batch_device: lens sum to {row0}, scores hold {scores_dev.numel()}")
    if kendall and "kendall" not in ent:
        # the Kendall side of the entry (a parallel descriptor array, the annotators' dense ranks), added the first time it is asked for:
        # Spearman calls on the same test set neither build nor read it
        for i, v in enumerate(videos):
            if not kendall_device_ready(v):
                raise _lib.SumkError(f"evaluate_batch_device: video {i} has {v['n_frames']} frames, the device Kendall kernel takes "
                                     f"{KENDALL_MAX_FRAMES}; use evaluate_batch")
        kd = (_lib.EvalDevKendall * n)()
        kmetas, users = [], 0
        for i, v in enumerate(videos):
            m = _device_meta(v, dev, kendall=True); kmetas.append(m)
            kd[i].y_dense, kd[i].ytie, kd[i].counts0 = m["ydense"].data_ptr(), m["ytie"].data_ptr(), users
            users += v["user_ranks"].shape[0]
        ent["kendall"] = dict(metas=kmetas, descr_dev=torch.frombuffer(bytearray(bytes(kd)), dtype=torch.uint8).to(dev), users=users,
                              per_video=[v["user_ranks"].shape[0] for v in videos])
    # Two stages on the device, two small transfers into pinned memory: the segment means come home after the short first kernel and the
    # host's key-shot selection + F-scores run while the device is still correlating (buffers are per batch and reused: the call ends
    # synchronised).
    # (the pinned buffers and events of an entry are shared by every call on that test set: calls from different threads / streams take
    #  turns -- ADVICE r4 -- instead of overwriting each other's results)
    import threading
    with ent.setdefault("lock", threading.Lock()):
        buf = ent.get("buffers")
        if buf is None:
            buf = ent["buffers"] = dict(
                scratch=torch.empty(frame0, dtype=torch.float32, device=dev), seg=torch.empty(max(seg0, 1), dtype=torch.float32, device=dev),
                corr=torch.empty(n, dtype=torch.float64, device=dev),
                part=torch.empty(max(1, lib.sumk_eval_device_spearman_scratch_bytes(n) // 8), dtype=torch.float64, device=dev),
                seg_host=torch.empty(max(seg0, 1), dtype=torch.float32).pin_memory(), corr_host=torch.empty(n, dtype=torch.float64).pin_memory(),
                ev_seg=torch.cuda.Event(), ev_corr=torch.cuda.Event())
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if select == "device":
            return _select_on_device(lib, ent, buf, videos, scores_dev, n, dev, st, proportion, method, want_summaries, kendall, counts_out)
        _lib.check(lib.sumk_eval_device_segments(scores_dev.data_ptr(), descr_dev.data_ptr(), n, buf["scratch"].data_ptr(), buf["seg"].data_ptr(), st),
                   "sumk_eval_device_segments")
        buf["seg_host"].copy_(buf["seg"], non_blocking=True); buf["ev_seg"].record()
        _enqueue_corr(lib, ent, buf, scores_dev, n, dev, st, kendall, counts_out, buf["corr"].data_ptr())
        buf["corr_host"].copy_(buf["corr"], non_blocking=True); buf["ev_corr"].record()
        seg_means = buf["seg_host"].numpy()[:seg0]       # (a view of the pinned buffer: valid once ev_seg has passed)
        arr = (_lib.EvalVideo * n)()
        summaries, seg_at = [], 0
        try:
            for i, v in enumerate(videos):
                e = arr[i]
                e.n_frames, e.n_steps = v["n_frames"], int(lens[i])
                e.cps, e.nfps, e.n_segs = v["cps"].ctypes.data, v["nfps"].ctypes.data, v["cps"].shape[0]
                e.seg_means = seg_means[seg_at:].ctypes.data
                seg_at += v["cps"].shape[0]
                e.corr = float("nan")             # (passed through untouched when seg_means is given; the device's value is returned below)
                if want_summaries:
                    o = np.empty(int(v["nfps"].sum()), dtype=np.float32); summaries.append(o); e.machine_summary = o.ctypes.data
                if "user_summary" in v:
                    if v["user_summary"].shape[1] != v["n_frames"]:
                        raise ValueError(f"user_summary has {v['user_summary'].shape[1]} frames, video has {v['n_frames']}")
                    e.user_summary, e.n_users = v["user_summary"].ctypes.data, v["user_summary"].shape[0]
            buf["ev_seg"].synchronize()
            _lib.check(lib.sumk_eval_videos(C.cast(arr, C.c_void_p), n, float(proportion), METHODS[method], int(n_threads)), "sumk_eval_videos")
        finally:
            buf["ev_corr"].synchronize()      # the call never returns with its pinned buffers still being written
        corr = buf["corr_host"].numpy().copy()
        if kendall and counts_out is not None:
            counts_out[:] = _split_counts(ent["kendall"]["buffers"]["counts_host"].numpy()[:4 * ent["kendall"]["users"]], ent["kendall"]["per_video"])
        f_avg = np.array([arr[i].f_avg for i in range(n)]); f_max = np.array([arr[i].f_max for i in range(n)])
    return corr, f_avg, f_max, (summaries if want_summaries else None)


def _enqueue_corr(lib, ent, buf, scores_dev, n, dev, st, kendall, counts_out, corr_ptr):
    """The correlation launch of a cached batch -- Spearman, or Kendall with its lazily built buffers and (counts_out given) the copy of
    the pair counts into pinned memory -- writing the n float64 results at corr_ptr.  Shared by both select modes."""
    import torch
    descr_dev = ent["descr_dev"]
    if kendall:
        kent = ent["kendall"]
        kbuf = kent.get("buffers")
        if kbuf is None:
            kbuf = kent["buffers"] = dict(
                tau=torch.empty(max(1, lib.sumk_eval_device_kendall_scratch_bytes(n, ent["frames"]) // 8), dtype=torch.float64, device=dev),
                counts=torch.empty(4 * max(kent["users"], 1), dtype=torch.int64, device=dev),
                counts_host=torch.empty(4 * max(kent["users"], 1), dtype=torch.int64).pin_memory())
        _lib.check(lib.sumk_eval_device_kendall(scores_dev.data_ptr(), descr_dev.data_ptr(), kent["descr_dev"].data_ptr(), n, kbuf["tau"].data_ptr(),
                                                corr_ptr, kbuf["counts"].data_ptr() if counts_out is not None else None, st),
                   "sumk_eval_device_kendall")
        if counts_out is not None:
            kbuf["counts_host"].copy_(kbuf["counts"], non_blocking=True)
    else:
        _lib.check(lib.sumk_eval_device_spearman(scores_dev.data_ptr(), descr_dev.data_ptr(), n, buf["part"].data_ptr(), corr_ptr, st),
                   "sumk_eval_device_spearman")


def _select_entry(lib, ent, buf, videos, n, dev, proportion, method):
    """The select side of a cached batch for one (proportion, method): descriptors (host + device copy) and device buffers, built the
    first time that pair is asked for.  `res` is the one block the call copies home: corr | f_avg | f_max | status (int32) per video."""
    import torch
    sel = ent.setdefault("select", {})
    key = (float(proportion), METHODS[method])
    se = sel.get(key)
    if se is not None:
        return se
    for i, v in enumerate(videos):
        if not select_device_ready(v, proportion):
            raise _lib.SumkError(f"evaluate_batch_device: video {i} does not qualify for select=\"device\" (needs <= {SELECT_MAX_SEGS} segments, "
                                 f"floor(n_frames x proportion) <= {SELECT_MAX_CAPACITY}, <= {SELECT_MAX_USERS} annotators over n_frames); "
                                 "use select=\"host\"")
    descr = (_lib.EvalDevSelect * n)()
    metas, at, seg_at = [], 0, 0
    for i, v in enumerate(videos):
        m = _device_meta(v, dev, select=True); metas.append(m)
        e = descr[i]
        e.seg_means, e.nfps = buf["seg"].data_ptr() + 4 * seg_at, m["nfps"].data_ptr()
        e.n_segs, e.n_frames, e.capacity = v["cps"].shape[0], v["n_frames"], select_capacity(v["n_frames"], proportion)
        e.summary_len, e.summary0, e.sel0 = int(v["nfps"].sum(dtype=np.int64)), at, seg_at
        if m["mask"] is not None:
            e.user_mask, e.n_users = m["mask"].data_ptr(), m["mask"].shape[0]
        e.method = METHODS[method]
        at += e.summary_len; seg_at += e.n_segs
    ws_bytes = lib.sumk_eval_device_select_workspace_bytes(n, max(e.n_segs for e in descr), max(e.capacity for e in descr))
    if ws_bytes == 0:
        raise _lib.SumkError("evaluate_batch_device: sumk_eval_device_select_workspace_bytes refused the batch")
    if len(sel) >= 4:
        sel.pop(next(iter(sel)))
    se = sel[key] = dict(
        metas=metas, descr=descr, descr_dev=torch.frombuffer(bytearray(bytes(descr)), dtype=torch.uint8).to(dev), summary_total=at,
        summary_lens=[e.summary_len for e in descr], summary=torch.empty(max(at, 1), dtype=torch.float32, device=dev),
        selected=torch.empty(max(seg_at, 1), dtype=torch.uint8, device=dev), res=torch.empty(4 * n, dtype=torch.float64, device=dev),
        ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev), res_host=torch.empty(4 * n, dtype=torch.float64).pin_memory(),
        summary_host=torch.empty(max(at, 1), dtype=torch.float32).pin_memory(), ev=torch.cuda.Event())
    return se


def _select_on_device(lib, ent, buf, videos, scores_dev, n, dev, st, proportion, method, want_summaries, kendall, counts_out):
    """evaluate_batch_device(select="device") behind the argument checks, under the entry's lock: three enqueues, one D2H, one wait."""
    se = _select_entry(lib, ent, buf, videos, n, dev, proportion, method)
    descr_dev, res = ent["descr_dev"], se["res"]
    _lib.check(lib.sumk_eval_device_segments(scores_dev.data_ptr(), descr_dev.data_ptr(), n, buf["scratch"].data_ptr(), buf["seg"].data_ptr(), st),
               "sumk_eval_device_segments")
    _lib.check(lib.sumk_eval_device_select(se["descr_dev"].data_ptr(), C.cast(se["descr"], C.c_void_p), n, se["summary"].data_ptr(), se["summary_total"],
                                           se["selected"].data_ptr(), ent["segs"], res.data_ptr() + 8 * n, res.data_ptr() + 16 * n,
                                           res.data_ptr() + 24 * n, se["ws"].data_ptr(), se["ws"].numel(), st), "sumk_eval_device_select")
    _enqueue_corr(lib, ent, buf, scores_dev, n, dev, st, kendall, counts_out, res.data_ptr())
    se["res_host"].copy_(res, non_blocking=True)
    if want_summaries:
        se["summary_host"].copy_(se["summary"], non_blocking=True)
    se["ev"].record()
    se["ev"].synchronize()
    home = se["res_host"].numpy()
    status = home[3 * n:].view(np.int32)[:n]
    if status.any():
        i = int(np.flatnonzero(status)[0])
        raise SelectStatusError(f"evaluate_batch_device: video {i}: sumk_eval_device_select status {int(status[i])} (1: a segment mean is not finite "
                             "or past 1e12; 2: segment values past the int32 profit rows; 3: n_frame_per_seg; 4: descriptor past the limits)")
    if kendall and counts_out is not None:
        counts_out[:] = _split_counts(ent["kendall"]["buffers"]["counts_host"].numpy()[:4 * ent["kendall"]["users"]], ent["kendall"]["per_video"])
    summaries = None
    if want_summaries:
        flat = se["summary_host"].numpy()[:se["summary_total"]]
        summaries = [a.copy() for a in np.split(flat, np.cumsum(se["summary_lens"])[:-1])]
    return home[:n].copy(), home[n:2 * n].copy(), home[2 * n:3 * n].copy(), summaries


# ---------------------------------------------------------------------------------------------- the long tail (csrc/evallong.hip, csrc/evalcorr_long.hip)
def select_long_device_ready(v, proportion):
    """select_device_ready with the frame budget of sumk_eval_device_select_long."""
    if "cps" not in v:
        return False
    nfps, us = v["nfps"], v.get("user_summary")
    if nfps.shape[0] != v["cps"].shape[0] or (nfps.shape[0] and (int(nfps.min()) < 0 or int(nfps.sum(dtype=np.int64)) >= 2 ** 31)):
        return False
    if us is not None and us.shape[1] != v["n_frames"]:
        return False
    return select_long_refusal(v["cps"].shape[0], v["n_frames"], 0 if us is None else us.shape[0], proportion) is None


def _long_entry(videos, lens, dev):
    """The cached side of evaluate_batch_device(tail="long") for one (videos, lens, device): checks, descriptors (host + device copy) and
    the buffers every metric and select mode share.  Kept under a key of its own beside the block tail's entry."""
    import torch
    key = (tuple(id(v) for v in videos), tuple(int(T) for T in lens), str(dev), "long")
    ent = _DEV_BATCH_CACHE.get(key)
    if ent is not None:
        return ent
    n = len(videos)
    for i, (v, T) in enumerate(zip(videos, lens)):
        if not device_ready_long(v):
            why = corr_long_refusal(v["picks"].shape[0], v["n_frames"], v["user_ranks"].shape[0]) if "user_ranks" in v else None
            raise _lib.SumkError(f"evaluate_batch_device: video {i} does not qualify for tail=\"long\" ({why or 'needs ascending picks, change points and annotator ranks over n_frames'}); "
                                 "use evaluate_batch")
        n_int = v["picks"].shape[0] - 1 + (1 if v["picks"][-1] != v["n_frames"] else 0)
        if n_int > int(T) + 1:
            raise _lib.SumkError(f"evaluate_batch_device: video {i} has {n_int} pick intervals for {int(T)} scores")
    descr = (_lib.EvalDevVideo * n)()
    metas, row0, frame0, seg0 = [], 0, 0, 0
    for i, (v, T) in enumerate(zip(videos, lens)):
        m = _device_meta(v, dev); metas.append(m)
        e = descr[i]
        e.picks, e.n_picks, e.n_frames, e.n_steps = m["picks"].data_ptr(), v["picks"].shape[0], v["n_frames"], int(T)
        e.row0, e.frame0 = row0, frame0
        e.cps, e.n_segs, e.seg0 = m["cps"].data_ptr(), v["cps"].shape[0], seg0
        e.user_ranks, e.user_mean, e.user_ssq, e.n_users = m["ranks"].data_ptr(), m["mean"].data_ptr(), m["ssq"].data_ptr(), v["user_ranks"].shape[0]
        row0 += int(T); frame0 += v["n_frames"]; seg0 += v["cps"].shape[0]
    if frame0 >= 2 ** 31 or row0 >= 2 ** 31:
        raise _lib.SumkError(f"evaluate_batch_device: the batch holds {frame0} frames and {row0} steps, the descriptors' offsets are int32")
    if len(_DEV_BATCH_CACHE) >= 8:
        _DEV_BATCH_CACHE.pop(next(iter(_DEV_BATCH_CACHE)))
    import threading
    ent = _DEV_BATCH_CACHE[key] = dict(videos=list(videos), metas=metas, descr=descr, descr_dev=torch.frombuffer(bytearray(bytes(descr)), dtype=torch.uint8).to(dev),
                                       rows=row0, frames=frame0, segs=seg0, lock=threading.Lock(), corr_ws={}, select={})
    return ent


def _evaluate_long(lib, videos, scores_dev, lens, proportion, method, want_summaries, n_threads, kendall, counts_out, select, max_workspace_bytes):
    """evaluate_batch_device(tail="long") behind the argument checks."""
    import torch
    from . import kts
    n, dev = len(videos), scores_dev.device
    ent = _long_entry(videos, lens, dev)
    descr, descr_dev, seg0 = ent["descr"], ent["descr_dev"], ent["segs"]
    if ent["rows"] != scores_dev.numel():
        raise _lib.SumkError(f"evaluate_batch_device: lens sum to {ent['rows']}, scores hold {scores_dev.numel()}")
    budget = kts.DEFAULT_MAX_WORKSPACE_BYTES if max_workspace_bytes is None else int(max_workspace_bytes)
    # ---- what the call needs, before anything is enqueued
    size_of = lib.sumk_eval_device_kendall_long_workspace_bytes if kendall else lib.sumk_eval_device_spearman_long_workspace_bytes
    corr_bytes = size_of(C.cast(descr, C.c_void_p), n)
    if corr_bytes == 0:
        raise _lib.SumkError("evaluate_batch_device: the long rank correlation refused the batch (a video past its limits)")
    sel_bytes = 0
    if select == "device":
        for i, v in enumerate(videos):
            if not select_long_device_ready(v, proportion):
                raise _lib.SumkError(f"evaluate_batch_device: video {i} does not qualify for select=\"device\" with tail=\"long\" (needs <= {SELECT_MAX_SEGS} "
                                     f"segments, floor(n_frames x proportion) <= {SELECT_LONG_MAX_CAPACITY}, <= {SELECT_MAX_USERS} annotators over n_frames); "
                                     "use select=\"host\"")
        sel_bytes = lib.sumk_eval_device_select_long_workspace_bytes(n, max(v["cps"].shape[0] for v in videos),
                                                                     max(select_capacity(v["n_frames"], proportion) for v in videos))
        if sel_bytes == 0:
            raise _lib.SumkError("evaluate_batch_device: sumk_eval_device_select_long_workspace_bytes refused the batch")
    if corr_bytes + sel_bytes > budget:
        raise _lib.SumkError(f"evaluate_batch_device(tail=\"long\"): the rank correlation needs a workspace of {corr_bytes} bytes and the selection one of "
                             f"{sel_bytes} bytes, {corr_bytes + sel_bytes} bytes together, over max_workspace_bytes={budget}; use evaluate_batch")
    with ent["lock"]:
        buf = ent.get("buffers")
        if buf is None:
            buf = ent["buffers"] = dict(
                scratch=torch.empty(ent["frames"], dtype=torch.float32, device=dev), seg=torch.empty(max(seg0, 1), dtype=torch.float32, device=dev),
                corr=torch.empty(n, dtype=torch.float64, device=dev), seg_host=torch.empty(max(seg0, 1), dtype=torch.float32).pin_memory(),
                corr_host=torch.empty(n, dtype=torch.float64).pin_memory(), ev_seg=torch.cuda.Event(), ev_corr=torch.cuda.Event())
        cw = ent["corr_ws"].get(kendall)
        if cw is None:
            cw = ent["corr_ws"][kendall] = dict(ws=torch.empty(corr_bytes, dtype=torch.uint8, device=dev))
            if kendall:
                kd = (_lib.EvalDevKendall * n)()
                kmetas, users = [], 0
                for i, v in enumerate(videos):
                    m = _device_meta(v, dev, kendall=True); kmetas.append(m)
                    kd[i].y_dense, kd[i].ytie, kd[i].counts0 = m["ydense"].data_ptr(), m["ytie"].data_ptr(), users
                    users += v["user_ranks"].shape[0]
                cw.update(metas=kmetas, descr_dev=torch.frombuffer(bytearray(bytes(kd)), dtype=torch.uint8).to(dev), users=users,
                          per_video=[v["user_ranks"].shape[0] for v in videos], counts=torch.empty(4 * max(users, 1), dtype=torch.int64, device=dev),
                          counts_host=torch.empty(4 * max(users, 1), dtype=torch.int64).pin_memory())
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        host_descr = C.cast(descr, C.c_void_p)

        def enqueue_corr(corr_ptr):
            if kendall:
                _lib.check(lib.sumk_eval_device_kendall_long(scores_dev.data_ptr(), descr_dev.data_ptr(), host_descr, cw["descr_dev"].data_ptr(), n,
                                                             cw["ws"].data_ptr(), cw["ws"].numel(), corr_ptr,
                                                             cw["counts"].data_ptr() if counts_out is not None else None, st), "sumk_eval_device_kendall_long")
                if counts_out is not None:
                    cw["counts_host"].copy_(cw["counts"], non_blocking=True)
            else:
                _lib.check(lib.sumk_eval_device_spearman_long(scores_dev.data_ptr(), descr_dev.data_ptr(), host_descr, n, cw["ws"].data_ptr(), cw["ws"].numel(),
                                                              corr_ptr, st), "sumk_eval_device_spearman_long")

        def counts_home():
            if kendall and counts_out is not None:
                counts_out[:] = _split_counts(cw["counts_host"].numpy()[:4 * cw["users"]], cw["per_video"])

        _lib.check(lib.sumk_eval_device_segments_long(scores_dev.data_ptr(), descr_dev.data_ptr(), host_descr, n, buf["scratch"].data_ptr(), buf["seg"].data_ptr(), st),
                   "sumk_eval_device_segments_long")
        if select == "device":
            se = _select_long_entry(ent, buf, videos, n, dev, proportion, method, sel_bytes)
            res = se["res"]
            _lib.check(lib.sumk_eval_device_select_long(se["descr_dev"].data_ptr(), C.cast(se["descr"], C.c_void_p), n, se["summary"].data_ptr(), se["summary_total"],
                                                        se["selected"].data_ptr(), ent["segs"], res.data_ptr() + 8 * n, res.data_ptr() + 16 * n,
                                                        res.data_ptr() + 24 * n, se["ws"].data_ptr(), se["ws"].numel(), st), "sumk_eval_device_select_long")
            enqueue_corr(res.data_ptr())
            se["res_host"].copy_(res, non_blocking=True)
            if want_summaries:
                se["summary_host"].copy_(se["summary"], non_blocking=True)
            se["ev"].record()
            se["ev"].synchronize()
            home = se["res_host"].numpy()
            status = home[3 * n:].view(np.int32)[:n]
            if status.any():
                i = int(np.flatnonzero(status)[0])
                raise SelectStatusError(f"evaluate_batch_device: video {i}: sumk_eval_device_select_long status {int(status[i])} (1: a segment mean is not "
                                        "finite or past 1e12; 2: segment values past the int32 profit rows; 3: n_frame_per_seg; 4: descriptor past the limits)")
            counts_home()
            summaries = None
            if want_summaries:
                flat = se["summary_host"].numpy()[:se["summary_total"]]
                summaries = [a.copy() for a in np.split(flat, np.cumsum(se["summary_lens"])[:-1])]
            return home[:n].copy(), home[n:2 * n].copy(), home[2 * n:3 * n].copy(), summaries
        # select="host": the segment means come home first, the host's selection and F-scores run under the correlation
        buf["seg_host"].copy_(buf["seg"], non_blocking=True); buf["ev_seg"].record()
        enqueue_corr(buf["corr"].data_ptr())
        buf["corr_host"].copy_(buf["corr"], non_blocking=True); buf["ev_corr"].record()
        seg_means = buf["seg_host"].numpy()[:seg0]
        arr = (_lib.EvalVideo * n)()
        summaries, seg_at = [], 0
        try:
            for i, v in enumerate(videos):
                e = arr[i]
                e.n_frames, e.n_steps = v["n_frames"], int(lens[i])
                e.cps, e.nfps, e.n_segs = v["cps"].ctypes.data, v["nfps"].ctypes.data, v["cps"].shape[0]
                e.seg_means = seg_means[seg_at:].ctypes.data
                seg_at += v["cps"].shape[0]
                e.corr = float("nan")
                if want_summaries:
                    o = np.empty(int(v["nfps"].sum()), dtype=np.float32); summaries.append(o); e.machine_summary = o.ctypes.data
                if "user_summary" in v:
                    if v["user_summary"].shape[1] != v["n_frames"]:
                        raise ValueError(f"user_summary has {v['user_summary'].shape[1]} frames, video has {v['n_frames']}")
                    e.user_summary, e.n_users = v["user_summary"].ctypes.data, v["user_summary"].shape[0]
            buf["ev_seg"].synchronize()
            _lib.check(lib.sumk_eval_videos(C.cast(arr, C.c_void_p), n, float(proportion), METHODS[method], int(n_threads)), "sumk_eval_videos")
        finally:
            buf["ev_corr"].synchronize()      # the call never returns with its pinned buffers still being written
        corr = buf["corr_host"].numpy().copy()
        counts_home()
        f_avg = np.array([arr[i].f_avg for i in range(n)]); f_max = np.array([arr[i].f_max for i in range(n)])
    return corr, f_avg, f_max, (summaries if want_summaries else None)


def _select_long_entry(ent, buf, videos, n, dev, proportion, method, ws_bytes):
    """_select_entry for sumk_eval_device_select_long: descriptors and device buffers of one (proportion, method) of a long entry."""
    import torch
    sel = ent["select"]
    key = (float(proportion), METHODS[method])
    se = sel.get(key)
    if se is not None:
        return se
    descr = (_lib.EvalDevSelect * n)()
    metas, at, seg_at = [], 0, 0
    for i, v in enumerate(videos):
        m = _device_meta(v, dev, select=True); metas.append(m)
        e = descr[i]
        e.seg_means, e.nfps = buf["seg"].data_ptr() + 4 * seg_at, m["nfps"].data_ptr()
        e.n_segs, e.n_frames, e.capacity = v["cps"].shape[0], v["n_frames"], select_capacity(v["n_frames"], proportion)
        e.summary_len, e.summary0, e.sel0 = int(v["nfps"].sum(dtype=np.int64)), at, seg_at
        if m["mask"] is not None:
            e.user_mask, e.n_users = m["mask"].data_ptr(), m["mask"].shape[0]
        e.method = METHODS[method]
        at += e.summary_len; seg_at += e.n_segs
    if len(sel) >= 4:
        sel.pop(next(iter(sel)))
    se = sel[key] = dict(
        metas=metas, descr=descr, descr_dev=torch.frombuffer(bytearray(bytes(descr)), dtype=torch.uint8).to(dev), summary_total=at,
        summary_lens=[e.summary_len for e in descr], summary=torch.empty(max(at, 1), dtype=torch.float32, device=dev),
        selected=torch.empty(max(seg_at, 1), dtype=torch.uint8, device=dev), res=torch.empty(4 * n, dtype=torch.float64, device=dev),
        ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev), res_host=torch.empty(4 * n, dtype=torch.float64).pin_memory(),
        summary_host=torch.empty(max(at, 1), dtype=torch.float32).pin_memory(), ev=torch.cuda.Event())
    return se
