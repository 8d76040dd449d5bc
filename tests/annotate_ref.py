"""Plain numpy specification of the dataset-record builder (include/sumk.h: sumk_annotate; summarizer_amd/utils/annotate.py): what the
fields of a trainable record are, given a video's raw annotations -- a helper module of the tests, in the role tests/kts_ref.py plays
for the change points.

The frame-level arithmetic is float32, one operation at a time in the order written here (the device unit is compiled without FMA
contraction, so every line below is one rounding there too).  Loops run over what the ORDER depends on -- the annotators of a frame, the
accumulators of a segment sum; along the frames the operations are element-wise and numpy applies them independently per element.  The
summaries come through the host `utils.eval.generate_summary`, which real-reference goldens pin (tests/golden/knapsack_e2e.npz,
tests/golden/annotate.npz); an annotator's frame-level row takes `arange(n_frames)` as its positions.  (Rank mode among EQUAL segment
scores: see `summary_and_flags`.)

protocol "scores"    (TVSum style: grades in [lo, hi]): user_scores, consensus, gtscore, seg_means, user_summary, gtsummary
protocol "summaries" (SumMe style: > 0 means selected): user_summary, consensus (the selection frequency), gtscore, user_scores, gtsummary"""
import math
import warnings

import numpy as np

from summarizer_amd.utils import eval as E

F32 = np.float32


def pairwise_sum(a):
    """numpy's float32 pairwise summation (numpy/core/src/umath/loops_utils.h.src) written out: below 8 elements a running sum, up to 128
    eight running accumulators combined as a tree and then the tail, above that two halves (the first a multiple of 8)."""
    a = np.asarray(a, dtype=F32)
    n = a.shape[0]
    if n < 8:
        r = F32(0)
        for i in range(n):
            r = F32(r + a[i])
        return r
    if n <= 128:
        r = a[:8].copy()
        i = 8
        while i < n - (n % 8):
            r = r + a[i:i + 8]                                  # eight independent float32 accumulators
            i += 8
        res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        while i < n:
            res = F32(res + a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F32(pairwise_sum(a[:n2]) + pairwise_sum(a[n2:]))


def segment_means(row, cps):
    """(n_segs,) float32: pairwise_sum(row[start .. end]) / (float)count, 0 for an empty segment (a pad segment of sumk_kts_segments)."""
    out = np.zeros(len(cps), dtype=F32)
    for s, (lo, hi) in enumerate(np.asarray(cps)[:, :2]):
        lo, hi = int(lo), int(hi) + 1
        if hi > lo:
            out[s] = F32(pairwise_sum(row[lo:hi]) / F32(hi - lo))
    return out


def scores_frame_level(anno, picks, cps, score_range=(1, 5)):
    """Protocol "scores" up to the selection: {"user_scores" (U, n_frames), "consensus" (n_frames,), "gtscore" (n_picks,),
    "seg_means" (U, n_segs)}, all float32."""
    anno = np.asarray(anno, dtype=F32)
    U, n_frames = anno.shape
    lo, hi = F32(score_range[0]), F32(score_range[1])
    span = F32(hi - lo)
    user_scores = ((anno - lo) / span).astype(F32)
    acc = np.zeros(n_frames, dtype=F32)
    for u in range(U):                                           # sequential over the annotators, from 0: NOT np.mean(axis=0)
        acc = (acc + anno[u]).astype(F32)
    consensus = (acc / F32(U)).astype(F32)
    g = consensus[np.asarray(picks, dtype=np.int64)]
    mn, mx = g.min(), g.max()
    gtscore = np.zeros(g.shape[0], dtype=F32) if mx == mn else ((g - mn) / F32(mx - mn)).astype(F32)
    seg_means = np.stack([segment_means(user_scores[u], cps) for u in range(U)])
    return {"user_scores": user_scores, "consensus": consensus, "gtscore": gtscore, "seg_means": seg_means}


def summaries_frame_level(anno, picks):
    """Protocol "summaries" up to the selection: {"user_summary" (U, n_frames) of 0 / 1, "consensus" (n_frames,) = the selection frequency,
    "gtscore" (n_picks,) = the frequency at the picks, not normalised}, all float32."""
    anno = np.asarray(anno, dtype=F32)
    U = anno.shape[0]
    on = anno > 0
    count = np.zeros(anno.shape[1], dtype=np.int32)
    for u in range(U):
        count += on[u]
    consensus = (count.astype(F32) / F32(U)).astype(F32)
    return {"user_summary": on.astype(F32), "consensus": consensus, "gtscore": consensus[np.asarray(picks, dtype=np.int64)].copy()}


def summary_and_flags(scores, cps, n_frames, nfps, positions, proportion=0.15, method="knapsack"):
    """The key-shot summary of utils.eval.generate_summary (float32 0 / 1 over sum(nfps) frames) and the (n_segs,) uint8 selection flags it
    expanded.  "knapsack" is generate_summary itself.  "rank" is generate_summary wherever that is defined: it walks `np.argsort(seg_score)
    [::-1]`, whose order among EQUAL scores is an accident of numpy's unstable default sort (it differs between CPUs), so equal scores are
    walked by the project's pinned rule -- descending score, the larger index first among equals, i.e. the stable ascending order from the
    back (csrc/evaltail.hip eval_one, tests/test_gpu_select.py) -- and the result is held to generate_summary whenever no two scores tie."""
    cps, nfps = np.asarray(cps), [int(x) for x in nfps]
    budget = int(math.floor(n_frames * proportion))
    with warnings.catch_warnings():                              # (numpy's mean of an EMPTY pad segment is NaN, with two warnings: such a
        warnings.simplefilter("ignore", RuntimeWarning)          #  segment holds no frame and is worth nothing to either method)
        return _summary_and_flags(scores, cps, n_frames, nfps, positions, proportion, method, budget)


def _summary_and_flags(scores, cps, n_frames, nfps, positions, proportion, method, budget):
    seg_score = E._segment_scores(E.upsample(scores, n_frames, positions), cps)
    if method == "rank":
        kept, used = [], 0
        for i in np.argsort(np.asarray(seg_score, dtype=np.float64), kind="stable")[::-1].tolist():
            if used + nfps[i] < budget:                          # strict, eval.py:105
                kept.append(i)
                used += nfps[i]
    else:
        kept = E._select_segments(seg_score, nfps, cps.shape[0], budget, method)
    flags = np.zeros(cps.shape[0], dtype=np.uint8)
    flags[np.asarray(kept, dtype=np.int64)] = 1
    summary = np.repeat(flags.astype(F32), nfps)
    if method != "rank" or len(set(seg_score)) == len(seg_score):
        assert np.array_equal(summary, E.generate_summary(scores, cps, n_frames, nfps, positions, proportion, method))
    return summary, flags


def record(anno, picks, n_frames, cps, nfps, protocol="scores", score_range=(1, 5), proportion=0.15, method="knapsack"):
    """Every annotation-derived field of one video's record, plus what the tests look at on the way: "consensus", "seg_means" (protocol
    "scores"), "gt_seg_means", "gt_frame_summary", "user_selected" (U, n_segs; protocol "scores") and "gt_selected" (n_segs,)."""
    picks = np.asarray(picks, dtype=np.int32)
    cps = np.asarray(cps, dtype=np.int32)
    n_frames = int(n_frames)
    if protocol == "scores":
        out = scores_frame_level(anno, picks, cps, score_range)
        rows = [summary_and_flags(out["user_scores"][u], cps, n_frames, nfps, np.arange(n_frames), proportion, method)
                for u in range(out["user_scores"].shape[0])]
        out["user_summary"] = np.stack([r[0] for r in rows])
        out["user_selected"] = np.stack([r[1] for r in rows])
    elif protocol == "summaries":
        out = summaries_frame_level(anno, picks)
        out["user_scores"] = E.upsample(out["gtscore"], n_frames, picks)[None, :]
    else:
        raise KeyError(f"Unknown protocol {protocol}")
    out["gt_seg_means"] = segment_means(E.upsample(out["gtscore"], n_frames, picks), cps)
    out["gt_frame_summary"], out["gt_selected"] = summary_and_flags(out["gtscore"], cps, n_frames, nfps, picks, proportion, method)
    out["gtsummary"] = out["gt_frame_summary"][picks.astype(np.int64)]
    return out


def block_grades(n_users, n_frames, seed, block=30):
    """TVSum-shaped annotations: integer grades 1 .. 5 held over blocks of `block` frames (many equal segment means: the tie rules)."""
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 6, size=(n_users, (n_frames + block - 1) // block)).astype(F32)
    return np.repeat(g, block, axis=1)[:, :n_frames].copy()


def block_selections(n_users, n_frames, seed, block=30, density=0.3):
    """SumMe-shaped annotations: 0 / positive values held over blocks of frames (any value > 0 means selected)."""
    rng = np.random.default_rng(seed)
    g = (rng.random((n_users, (n_frames + block - 1) // block)) < density) * rng.integers(1, 4, size=(n_users, (n_frames + block - 1) // block))
    return np.repeat(g.astype(F32), block, axis=1)[:, :n_frames].copy()


def segments_of_lengths(lengths, n_pad=0):
    """((S + n_pad, 2) int32 change points, (S + n_pad,) int32 frames per segment) for consecutive segments of the given lengths, followed by
    n_pad EMPTY segments (n_frames, n_frames - 1) as sumk_kts_segments pads them."""
    lengths = np.asarray(lengths, dtype=np.int64)
    ends = np.cumsum(lengths) - 1
    starts = ends - lengths + 1
    n_frames = int(lengths.sum())
    cps = np.concatenate([np.stack([starts, ends], axis=1), np.tile([[n_frames, n_frames - 1]], (n_pad, 1))]).astype(np.int32)
    return cps, np.concatenate([lengths, np.zeros(n_pad, dtype=np.int64)]).astype(np.int32)
