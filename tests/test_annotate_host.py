"""CPU: the specification of the dataset-record builder (tests/annotate_ref.py) against the real-reference golden and against cases
small enough to compute by hand, and everything `summarizer_amd.utils.annotate.build_records` refuses on the host before it touches the
GPU.  Every comparison is exact: the arithmetic is specified operation for operation."""
import ctypes as C

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import annotate_ref as A
from summarizer_amd import _lib
from summarizer_amd._lib import SumkError
from summarizer_amd.utils import annotate as M
from summarizer_amd.utils import eval as E

F32 = np.float32


@pytest.fixture(scope="module")
def gold(golden):
    return golden("annotate")


def test_pairwise_sum_is_numpys():
    """The written-out tree is numpy's own float32 summation at every size where it changes shape (8, 128, the halves above)."""
    rng = np.random.default_rng(1)
    for n in (0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1000, 4494):
        a = rng.random(n).astype(F32)
        assert A.pairwise_sum(a) == a.sum(dtype=F32), n
        if n:
            assert F32(A.pairwise_sum(a) / F32(n)) == a.mean(), n
    row = rng.random(611).astype(F32)
    cps, _ = A.segments_of_lengths([1, 7, 8, 9, 128, 129, 329], n_pad=2)
    want = np.array(E._segment_scores(row, cps[:-2]), dtype=F32)
    assert_array_equal(A.segment_means(row, cps), np.concatenate([want, [0, 0]]).astype(F32))


def test_spec_equals_golden_scores_rank(gold):
    r = A.record(gold["anno_scores"], gold["picks"], int(gold["n_frames"]), gold["change_points"], gold["n_frame_per_seg"], "scores", (1, 5), 0.15, "rank")
    assert_array_equal(r["user_summary"], gold["scores/user_summary_rank"])
    assert_array_equal(r["gtsummary"], gold["scores/gtsummary_rank"])
    assert r["user_summary"].dtype == F32 and r["gtsummary"].dtype == F32 and r["user_summary"].sum() > 0


def test_spec_equals_golden_summaries(gold):
    r = A.record(gold["anno_summaries"], gold["picks"], int(gold["n_frames"]), gold["change_points"], gold["n_frame_per_seg"], "summaries", (1, 5), 0.15, "rank")
    assert_array_equal(r["user_scores"], gold["summaries/user_scores"])
    assert_array_equal(r["gtsummary"], gold["summaries/gtsummary_rank"])
    assert_array_equal(r["user_summary"], (gold["anno_summaries"] > 0).astype(F32))
    assert r["user_scores"].shape == (1, int(gold["n_frames"]))


def test_rank_ties_follow_the_pinned_rule():
    """Equal scores: descending score, the larger index first among equals, strict budget -- and generate_summary itself where nothing ties."""
    cps, nfps = A.segments_of_lengths([10, 10, 10, 10])
    scores = np.repeat(np.array([0.5, 0.25, 0.5, 0.25], F32), 10)
    summary, flags = A.summary_and_flags(scores, cps, 40, nfps, np.arange(40), proportion=0.3, method="rank")      # budget 12: one segment of 10
    assert_array_equal(flags, [0, 0, 1, 0])
    assert_array_equal(summary, np.repeat(np.array([0, 0, 1, 0], F32), 10))
    scores = np.repeat(np.array([0.5, 0.25, 0.75, 0.125], F32), 10)
    summary, flags = A.summary_and_flags(scores, cps, 40, nfps, np.arange(40), proportion=0.6, method="rank")      # budget 24: two segments
    assert_array_equal(flags, [1, 0, 1, 0])
    assert_array_equal(summary, E.generate_summary(scores, cps, 40, nfps.tolist(), np.arange(40), 0.6, "rank"))


def test_one_annotator_by_hand():
    cps, nfps = A.segments_of_lengths([2, 2])
    r = A.record(np.array([[1, 3, 5, 5]], F32), np.arange(4), 4, cps, nfps, "scores", (1, 5), 0.5, "knapsack")
    assert_array_equal(r["user_scores"], np.array([[0, 0.5, 1, 1]], F32))
    assert_array_equal(r["consensus"], np.array([1, 3, 5, 5], F32))
    assert_array_equal(r["gtscore"], np.array([0, 0.5, 1, 1], F32))
    assert_array_equal(r["seg_means"], np.array([[0.25, 1]], F32))
    assert_array_equal(r["gt_seg_means"], np.array([0.25, 1], F32))
    assert_array_equal(r["user_summary"], np.array([[0, 0, 1, 1]], F32))        # budget 2 frames: the segment worth 1000 beats the one worth 250
    assert_array_equal(r["user_selected"], np.array([[0, 1]], np.uint8))
    assert_array_equal(r["gtsummary"], np.array([0, 0, 1, 1], F32))


def test_consensus_is_the_sequential_sum():
    """Three annotators whose float32 sum depends on the order: ((a + b) + c) / 3, from 0."""
    a = np.array([[1e8], [1.0], [-1e8]], F32)
    cps, nfps = A.segments_of_lengths([1])
    r = A.scores_frame_level(a, [0], cps, (0, 1))
    assert_array_equal(r["consensus"], np.array([F32(F32(F32(F32(0) + a[0, 0]) + a[1, 0]) + a[2, 0]) / F32(3)], F32))
    assert r["consensus"][0] == 0 and F32(F32(a[0, 0] + a[2, 0]) + a[1, 0]) == 1


def test_constant_video_by_hand():
    cps, nfps = A.segments_of_lengths([5, 9, 6])
    r = A.record(np.full((2, 20), 3, F32), [0, 7, 14], 20, cps, nfps, "scores", (1, 5), 0.5, "knapsack")
    assert_array_equal(r["user_scores"], np.full((2, 20), 0.5, F32))
    assert_array_equal(r["consensus"], np.full(20, 3, F32))
    assert_array_equal(r["gtscore"], np.zeros(3, F32))                           # max == min: all zeros, no 0 / 0
    assert_array_equal(r["seg_means"], np.full((2, 3), 0.5, F32))
    assert_array_equal(r["gt_seg_means"], np.zeros(3, F32))
    assert_array_equal(r["user_summary"], np.stack([E.generate_summary(np.full(20, 0.5, F32), cps, 20, nfps.tolist(), np.arange(20), 0.5)] * 2))
    assert r["gtsummary"].shape == (3,)


def test_one_segment_video_by_hand():
    """A single segment as long as the video never fits the budget: empty summaries.  Protocol "summaries": any value > 0 is a selection."""
    cps, nfps = A.segments_of_lengths([4])
    anno = np.array([[0, 2, 0, 1], [0, 1, 0, 0], [0, 0, -1, 3]], F32)
    r = A.record(anno, [1, 3], 4, cps, nfps, "summaries", (1, 5), 0.15, "knapsack")
    assert_array_equal(r["user_summary"], np.array([[0, 1, 0, 1], [0, 1, 0, 0], [0, 0, 0, 1]], F32))
    two_thirds = F32(F32(2) / F32(3))
    assert_array_equal(r["consensus"], np.array([0, two_thirds, 0, two_thirds], F32))
    assert_array_equal(r["gtscore"], np.array([two_thirds, two_thirds], F32))    # not normalised
    assert_array_equal(r["user_scores"], np.array([[0, two_thirds, two_thirds, two_thirds]], F32))     # nothing in front of the first pick
    assert_array_equal(r["gt_frame_summary"], np.zeros(4, F32))
    assert_array_equal(r["gtsummary"], np.zeros(2, F32))
    r = A.record(np.array([[1, 5, 2, 2]], F32), [0, 1, 2, 3], 4, cps, nfps, "scores", (1, 5), 0.15, "rank")
    assert_array_equal(r["user_summary"], np.zeros((1, 4), F32))
    assert_array_equal(r["gtscore"], np.array([0, 1, 0.25, 0.25], F32))


# ------------------------------------------------------------------------------------------------ the binding and the host-side refusals
def test_abi_of_the_new_entries():
    assert C.sizeof(_lib.AnnotateVideo) == 88            # three pointers, six int32, five int64
    lib = _lib.load()
    for name in ("sumk_annotate", "sumk_annotate_gtsummary"):
        assert hasattr(lib, name) and name in _lib._SIGS
    assert M.MAX_PICKS == 4095 and M.MAX_USERS == 32 and M.MAX_SEGS == 1024 and M.PROTOCOLS == {"scores": 0, "summaries": 1}


def _video(n_frames=60, U=3, T=4, **over):
    v = {"features": np.ones((T, 8), F32), "picks": (np.arange(T) * (n_frames // T)).astype(np.int32), "n_frames": n_frames,
         "annotations": np.full((U, n_frames), 2, F32), "change_points": np.array([[0, n_frames // 2 - 1], [n_frames // 2, n_frames - 1]], np.int32),
         "n_frame_per_seg": np.array([n_frames // 2, n_frames - n_frames // 2], np.int32)}
    v.update(over)
    return {k: x for k, x in v.items() if x is not None}


# name: (what the bad video differs in, the text of ITS refusal)
REFUSALS = {
    "no annotations": (dict(annotations=None), "video bad has no `annotations`"),
    "no picks": (dict(picks=None), "video bad has no `picks`"),
    "features not 2-d": (dict(features=np.ones(4, F32)), r"video bad: features must be \(n_steps, D\)"),
    "picks per step": (dict(picks=np.arange(5, dtype=np.int32)), "video bad: picks must be 4 integers"),
    "float picks": (dict(picks=np.arange(4, dtype=np.float32)), "video bad: picks must be 4 integers"),
    "picks descend": (dict(picks=np.array([0, 30, 15, 45], np.int32)), "video bad: picks must ascend inside 0 .. n_frames - 1 = 59"),
    "pick negative": (dict(picks=np.array([-1, 15, 30, 45], np.int32)), "video bad: picks must ascend inside"),
    "pick past the video": (dict(picks=np.array([0, 15, 30, 60], np.int32)), "video bad: picks must ascend inside"),
    "annotations span": (dict(annotations=np.ones((3, 59), F32)), r"video bad: annotations must be \(n_users, n_frames = 60\)"),
    "annotations 1-d": (dict(annotations=np.ones(60, F32)), r"video bad: annotations must be \(n_users"),
    "annotations not finite": (dict(annotations=np.full((3, 60), np.nan, F32)), "video bad: annotations must be finite"),
    "one infinite annotation": (dict(annotations=np.where(np.arange(180).reshape(3, 60) == 77, np.inf, 2).astype(F32)), "video bad: annotations must be finite"),
    "33 annotators": (dict(annotations=np.ones((33, 60), F32)), r"video bad has 33 annotators \(1 .. 32\)"),
    "no annotators": (dict(annotations=np.ones((0, 60), F32)), r"video bad has 0 annotators \(1 .. 32\)"),
    "4096 picks": (dict(n_frames=5000, features=np.ones((4096, 8), F32), picks=np.arange(4096, dtype=np.int32), annotations=np.ones((2, 5000), F32),
                       change_points=np.array([[0, 4999]], np.int32), n_frame_per_seg=np.array([5000], np.int32)),
                   r"video bad has 4096 picks \(1 .. 4095\)"),
    "1025 segments": (dict(n_frames=2050, annotations=np.ones((2, 2050), F32), picks=np.arange(4, dtype=np.int32),
                          change_points=np.stack([2 * np.arange(1025), 2 * np.arange(1025) + 1], axis=1).astype(np.int32),
                          n_frame_per_seg=np.full(1025, 2, np.int32)), r"video bad has 1025 segments \(1 .. 1024\)"),
    "budget past 8191": (dict(n_frames=54614, annotations=np.ones((1, 54614), F32), picks=np.arange(4, dtype=np.int32),
                             change_points=np.array([[0, 54613]], np.int32), n_frame_per_seg=np.array([54614], np.int32)),
                         "video bad has a budget of 8192 frames"),
    "segments short of the video": (dict(n_frame_per_seg=np.array([30, 29], np.int32), change_points=np.array([[0, 29], [30, 58]], np.int32)),
                                    r"video bad: the segments must tile the video's 60 frames \(n_frame_per_seg sums to 59\)"),
    "segments disagree with their lengths": (dict(n_frame_per_seg=np.array([20, 40], np.int32)), "video bad: the segments must tile"),
    "negative segment length": (dict(n_frame_per_seg=np.array([70, -10], np.int32), change_points=np.array([[0, 69], [70, 59]], np.int32)),
                                "video bad: the segments must tile"),
    "change points without lengths": (dict(n_frame_per_seg=None), "video bad: change_points and n_frame_per_seg come together"),
    "lengths without change points": (dict(change_points=None), "video bad: change_points and n_frame_per_seg come together"),
    "segment counts differ": (dict(n_frame_per_seg=np.array([60], np.int32)), "video bad: change_points .* and n_frame_per_seg .* do not match"),
}


class _ReachedTheGpu(Exception):
    pass


def _tripwires(monkeypatch):
    """A machine with a GPU, as far as build_records can tell, on which any upload or chain construction raises _ReachedTheGpu."""
    def reached(*a, **k):
        raise _ReachedTheGpu()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(M, "AnnotateChain", reached)
    monkeypatch.setattr(torch, "from_numpy", reached)


def test_valid_videos_pass_every_host_check(monkeypatch):
    """The control of the refusals below: the same videos without a defect get as far as the first upload -- with and without change
    points, equal neighbouring picks included."""
    _tripwires(monkeypatch)
    with pytest.raises(_ReachedTheGpu):
        M.build_records({"good": _video(), "bad": _video()})
    with pytest.raises(_ReachedTheGpu):
        M.build_records({"a": _video(change_points=None, n_frame_per_seg=None), "b": _video(picks=np.array([0, 15, 15, 59], np.int32))}, protocol="summaries")


def test_build_records_without_a_gpu_says_so(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(M, "AnnotateChain", None)
    with pytest.raises(SumkError, match="no GPU"):
        M.build_records({"good": _video()})


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_build_records_refuses_on_the_host(name, monkeypatch):
    """Everything only Python can see is refused with SumkError -- the refusal of THAT defect, naming the video -- BEFORE anything is
    uploaded or enqueued (a GPU is reported present, so no other SumkError stands in; test_valid_videos_pass_every_host_check is the control)."""
    _tripwires(monkeypatch)
    over, text = REFUSALS[name]
    with pytest.raises(SumkError, match=text):
        M.build_records({"good": _video(), "bad": _video(**over)})


def test_build_records_refuses_options(monkeypatch):
    _tripwires(monkeypatch)
    vids = {"v": _video()}
    with pytest.raises(KeyError, match="protocol"):
        M.build_records(vids, protocol="grades")
    with pytest.raises(KeyError, match="method"):
        M.build_records(vids, method="greedy")
    with pytest.raises(TypeError, match="KTS"):
        M.build_records(vids, max_cps=3)
    for bad in ((5, 5), (5, 1), (1, np.inf), (np.nan, 5), (1, 1 + 1e-9)):
        with pytest.raises(SumkError, match="score_range"):
            M.build_records(vids, score_range=bad)
    with pytest.raises(SumkError, match="feature size"):
        M.build_records({"a": _video(change_points=None, n_frame_per_seg=None), "b": _video(features=np.ones((4, 12), F32), change_points=None,
                                                                                               n_frame_per_seg=None)})
    assert len(M.build_records({})) == 0


def test_refusal_names_the_limit():
    assert M.refusal(20, 4494, 300, 40, 0.15) is None
    assert "annotators" in M.refusal(33, 100, 10, 2, 0.15) and "annotators" in M.refusal(0, 100, 10, 2, 0.15)
    assert "picks" in M.refusal(3, 5000, 4096, 2, 0.15) and "picks" in M.refusal(3, 100, 0, 2, 0.15)
    assert "segments" in M.refusal(3, 5000, 10, 1025, 0.15) and "budget" in M.refusal(3, 54614, 10, 2, 0.15)
    assert "frames" in M.refusal(3, (1 << 24) + 1, 10, 2, 0.0001)


# ------------------------------------------------------------------------------------------------ what sumk_annotate refuses on the host copy
def _c_entry(descr, protocol=0, lo=1.0, hi=5.0, totals=(1 << 40,) * 4, fake=0x1000):
    """sumk_annotate with made-up non-null pointers, for calls that are REFUSED: every check is made on the host copy of the descriptors,
    before any HIP call, so the answer needs no GPU and nothing is launched.  Never pass arguments that would be accepted: on a machine
    with a GPU the kernels would run on these addresses (the accepted side of each limit is in tests/test_gpu_annotate.py, on real buffers)."""
    lib = _lib.load()
    rc = lib.sumk_annotate(fake, C.cast(descr, C.c_void_p), len(descr), protocol, lo, hi, fake, totals[0], fake, totals[1], fake, totals[2], fake, totals[3], None)
    return rc, lib.sumk_last_error().decode(errors="replace")


def _descriptors(n, n_frames=60, **over):
    d = (_lib.AnnotateVideo * n)()
    for e in d:
        e.anno = e.picks = e.cps = 0x1000
        e.n_users, e.n_frames, e.n_picks, e.n_segs, e.summary_len = 3, n_frames, 4, 2, n_frames
        for k, v in over.items():
            setattr(e, k, v)
    return d


def test_c_entry_refuses_on_the_host_copy():
    for over, text in ((dict(reserved=1), "reserved"), (dict(n_users=33), "33 annotators"), (dict(n_picks=4096), "4096 picks"), (dict(n_segs=1025), "1025 segments"),
                       (dict(summary_len=59), "tile"), (dict(n_frames=(1 << 24) + 1, summary_len=(1 << 24) + 1), "frames"), (dict(anno=None), "null"),
                       (dict(user0=-1), "rows"), (dict(pick0=1 << 41), "picks")):
        rc, err = _c_entry(_descriptors(2, **over))
        assert rc == -1 and text in err, (over, err)
    assert _c_entry(_descriptors(1), hi=1.0)[0] == -1 and _c_entry(_descriptors(1), protocol=2)[0] == -1
    # a frame pass past one launch: ceil(2^24 / 256) blocks per video x 256 videos = 2^24 blocks of 256 threads = 2^32 threads
    rc, err = _c_entry(_descriptors(256, n_frames=1 << 24))
    assert rc == -1 and "split the batch" in err, err
    rc, err = _c_entry(_descriptors(65536, n_frames=257))
    assert rc == -1 and "65536 videos" in err, err
