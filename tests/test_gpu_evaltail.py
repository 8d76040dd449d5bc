"""Device-side evaluation tail (csrc/evaldev.hip): upsample + float32 segment means + Spearman on the GPU with the
scores still in HBM, key-shot selection / F-scores finished on the host -- against the all-host native tail (which test_host_eval.py
holds bit-exact to the numpy specification and to the reference's goldens).  The second half runs recipes.eval_edge_batch (the geometries a
plain synthetic video never has), compares the Spearman values with scipy and the segment means with numpy as well, and drives the one-launch
entry sumk_eval_device and the over-limit guard of all three C entries."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import recipes as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method", ["knapsack", "rank"])
def test_device_tail_equals_host_tail(method):
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    vids, scores, lens = [], [], []
    for i, (T, U) in enumerate([(300, 15), (1, 3), (97, 20), (650, 18), (33, 5), (320, 32), (150, 1)]):
        v = R.synthetic_video(T, 8100 + i, n_users=U)
        s = rng.random(T).astype(np.float32)
        if i == 2:
            s[10:40] = s[10]                                   # long runs of EQUAL step scores: tie groups across pick intervals
        if i == 4:
            s[:] = 0.25                                        # every frame tied
        vids.append(eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"],
                                              E.rank_users(v["user_scores"])))
        scores.append(s); lens.append(T)
        assert eval_native.device_ready(vids[-1])
    want = eval_native.evaluate_batch(vids, scores, 0.15, method, want_summaries=True, n_threads=3)
    packed = torch.from_numpy(np.concatenate(scores)).to(dev)
    got = eval_native.evaluate_batch_device(vids, packed, lens, 0.15, method, want_summaries=True, n_threads=3)
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-12)          # Spearman: float64, different summation order
    np.testing.assert_array_equal(got[1], want[1])                           # F-scores: bit-identical (same integers into the knapsack)
    np.testing.assert_array_equal(got[2], want[2])
    for a, b in zip(got[3], want[3]):
        np.testing.assert_array_equal(a, b)
    # the batch's descriptors, device buffers and pinned buffers are kept between calls (Trainer.test asks for the same fold every time):
    # other scores for the same videos, then a sub-batch of them, still give the host tail's numbers
    scores2 = [rng.random(T).astype(np.float32) for T in lens]
    want2 = eval_native.evaluate_batch(vids, scores2, 0.15, method, n_threads=3)
    got2 = eval_native.evaluate_batch_device(vids, torch.from_numpy(np.concatenate(scores2)).to(dev), lens, 0.15, method, n_threads=3)
    np.testing.assert_allclose(got2[0], want2[0], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got2[1], want2[1]); np.testing.assert_array_equal(got2[2], want2[2])
    assert not np.array_equal(got2[0], got[0])
    sub = [0, 3, 5]
    want3 = eval_native.evaluate_batch([vids[i] for i in sub], [scores2[i] for i in sub], 0.15, method, n_threads=3)
    got3 = eval_native.evaluate_batch_device([vids[i] for i in sub], torch.from_numpy(np.concatenate([scores2[i] for i in sub])).to(dev),
                                             [lens[i] for i in sub], 0.15, method, n_threads=3)
    np.testing.assert_allclose(got3[0], want3[0], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got3[1], want3[1]); np.testing.assert_array_equal(got3[2], want3[2])


def test_device_tail_declines_what_it_does_not_cover():
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    v = R.synthetic_video(60, 8200, n_users=4)
    ok = eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"], E.rank_users(v["user_scores"]))
    assert eval_native.device_ready(ok)
    shuffled = eval_native.prepare_video(v["n_frames"], v["picks"][::-1].copy(), v["change_points"], v["n_frame_per_seg"], v["user_summary"],
                                         E.rank_users(v["user_scores"]))
    assert not eval_native.device_ready(shuffled)                            # picks not ascending -> host tail
    assert not eval_native.device_ready(eval_native.prepare_video(v["n_frames"], v["picks"]))          # no change points / ranks


# ------------------------------------------------------------------------------------------------ the edge batch (recipes.eval_edge_batch)
# tests/test_oracle.py holds the host tail on this batch bit-exact (summaries, F-scores) / to 1e-12 (Spearman) against the numpy oracle.

def _prepare(v):
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    return eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"],
                                     E.rank_users(v["user_scores"]))


def _descriptors(vids, lens, dev, override=None):
    """Device descriptors built the way evaluate_batch_device builds them.  override: {video index: {field: value}} applied on top."""
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    descr = (_lib.EvalDevVideo * len(vids))()
    row0 = frame0 = seg0 = 0
    keep = []
    for i, (v, T) in enumerate(zip(vids, lens)):
        m = eval_native._device_meta(v, dev); keep.append(m)
        e = descr[i]
        e.picks, e.n_picks, e.n_frames, e.n_steps = m["picks"].data_ptr(), v["picks"].shape[0], v["n_frames"], int(T)
        e.row0, e.frame0 = row0, frame0
        e.cps, e.n_segs, e.seg0 = m["cps"].data_ptr(), v["cps"].shape[0], seg0
        e.user_ranks, e.user_mean, e.user_ssq, e.n_users = m["ranks"].data_ptr(), m["mean"].data_ptr(), m["ssq"].data_ptr(), v["user_ranks"].shape[0]
        for k, val in (override or {}).get(i, {}).items():
            setattr(e, k, val)
        row0 += int(T); frame0 += v["n_frames"]; seg0 += v["cps"].shape[0]
    descr_dev = torch.frombuffer(bytearray(bytes(descr)), dtype=torch.uint8).to(dev)
    return descr_dev, keep, row0, frame0, seg0


def _c_entries(vids, lens, scores_dev, override=None):
    """The three C entries on buffers of the test's own, every one of them filled with 0xFF bytes first.
    Returns (segment means of sumk_eval_device_segments, correlations of sumk_eval_device_spearman, both of the one-launch sumk_eval_device)."""
    from summarizer_amd import _lib
    lib = _lib.load()
    dev, n = scores_dev.device, len(vids)
    descr_dev, keep, rows, frames, segs = _descriptors(vids, lens, dev, override)
    assert rows <= scores_dev.numel()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def poisoned(numel, dtype):
        t = torch.empty(numel, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(255)
        return t
    scratch, seg2, corr2 = poisoned(frames, torch.float32), poisoned(segs, torch.float32), poisoned(n, torch.float64)
    part = poisoned(lib.sumk_eval_device_spearman_scratch_bytes(n) // 8, torch.float64)
    _lib.check(lib.sumk_eval_device_segments(scores_dev.data_ptr(), descr_dev.data_ptr(), n, scratch.data_ptr(), seg2.data_ptr(), st), "segments")
    _lib.check(lib.sumk_eval_device_spearman(scores_dev.data_ptr(), descr_dev.data_ptr(), n, part.data_ptr(), corr2.data_ptr(), st), "spearman")
    scratch1, seg1, corr1 = poisoned(frames, torch.float32), poisoned(segs, torch.float32), poisoned(n, torch.float64)
    _lib.check(lib.sumk_eval_device(scores_dev.data_ptr(), descr_dev.data_ptr(), n, scratch1.data_ptr(), seg1.data_ptr(), corr1.data_ptr(), st), "eval_device")
    torch.cuda.synchronize(dev)
    return seg2.cpu().numpy(), corr2.cpu().numpy(), seg1.cpu().numpy(), corr1.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _oracle(batch):
    """Per video: (Spearman of scipy's rankdata + spearmanr on the oracle's upsampled scores, float32 segment means of numpy's mean).
    A change point that starts below 0 is clamped for the oracle (numpy's slice would wrap: see tests/test_oracle.py)."""
    from oracle import eval_np
    corr, seg = [], []
    for name, v, s in batch:
        fs = eval_np.upsample(s, v["n_frames"], v["picks"])
        with np.errstate(invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            corr.append(float(eval_np.evaluate_scores(fs, v["user_scores"])))
        cps = v["change_points"].copy()
        if name == "cps_start_below_0":
            cps[0, 0] = 0
        assert cps.min() >= 0
        seg.append(np.asarray(eval_np.segment_scores(fs, cps), dtype=np.float32))
    return np.asarray(corr), seg


def _check_against_oracle(what, corr_dev, corr_host, corr_ref):
    """Device Spearman vs the independent definition: 4 x the host tail's own distance from the oracle on these videos, floor 1e-12."""
    nan = np.isnan(corr_ref)
    assert np.array_equal(np.isnan(corr_dev), nan), (what, corr_dev, corr_ref)
    host = float(np.abs(corr_host[~nan] - corr_ref[~nan]).max())
    got = float(np.abs(corr_dev[~nan] - corr_ref[~nan]).max())
    print(f"EVALTAIL {what}: max |device - oracle| = {got:.3e}, max |host tail - oracle| = {host:.3e}, NaN videos = {int(nan.sum())}")
    assert got <= max(4 * host, 1e-12), (what, got, host)
    return int(nan.sum())


def _cache_entry(vids, lens, dev):
    from summarizer_amd.utils import eval_native
    return eval_native._DEV_BATCH_CACHE.get((tuple(id(v) for v in vids), tuple(int(T) for T in lens), str(dev)))


@pytest.mark.parametrize("method", ["knapsack", "rank"])
def test_device_tail_on_the_edge_batch(method):
    """Frames in front of the first pick (and their tie with intervals that score exactly 0), picks[-1] == n_frames, repeated picks, one
    interval more than scores, change points outside the video, segments of 1 .. 1100 frames, 4000 / 4095 / 4096 intervals, videos of 1, 5
    and 9 frames, negative scores and -0.0; 1, 2, 31 and 32 annotators: against the host tail under this file's rules, the Spearman values
    also against scipy, the segment means bit for bit against numpy's float32 mean; the same bits again after the cached device buffers were
    filled with 0xFF bytes; and the one-launch entry sumk_eval_device against the two-launch form."""
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    batch = R.eval_edge_batch()
    vids = [_prepare(v) for _, v, _ in batch]
    scores, lens = [s for _, _, s in batch], [v["n_steps"] for _, v, _ in batch]
    assert all(eval_native.device_ready(v) for v in vids)
    assert {v["user_ranks"].shape[0] for v in vids} == {1, 2, 31, 32}
    want = eval_native.evaluate_batch(vids, scores, 0.15, method, want_summaries=True, n_threads=3)
    packed = torch.from_numpy(np.concatenate(scores)).to(dev)
    got = eval_native.evaluate_batch_device(vids, packed, lens, 0.15, method, want_summaries=True, n_threads=3)
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-12)          # (NaN == NaN here: assert_allclose's equal_nan default)
    assert np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    for a, b in zip(got[3], want[3]):
        np.testing.assert_array_equal(a, b)
    corr_ref, seg_ref = _oracle(batch)
    assert _check_against_oracle("evaluate_batch_device", got[0], want[0], corr_ref) == 2      # n_frames_1 and all_zero+picks_from_7 (asserted on the oracle in _check)
    assert np.isnan(corr_ref).sum() <= 2
    # the same bits with every cached device buffer poisoned
    ent = _cache_entry(vids, lens, dev)
    assert ent is not None
    seg_dev = ent["buffers"]["seg_host"].numpy()[:ent["segs"]].copy()
    for k in ("scratch", "seg", "corr", "part"):
        ent["buffers"][k].view(torch.uint8).fill_(255)
    again = eval_native.evaluate_batch_device(vids, packed, lens, 0.15, method, want_summaries=True, n_threads=3)
    assert np.array_equal(_bits(again[0]), _bits(got[0])) and np.array_equal(_bits(again[1]), _bits(got[1])) and np.array_equal(_bits(again[2]), _bits(got[2]))
    for a, b in zip(again[3], got[3]):
        np.testing.assert_array_equal(a, b)
    assert np.array_equal(_bits(ent["buffers"]["seg_host"].numpy()[:ent["segs"]]), _bits(seg_dev))
    # segment means: numpy's pairwise float32 mean, bit for bit (an all -0.0 segment, whose sign of zero no consumer sees, is not in the batch)
    assert np.array_equal(_bits(seg_dev), _bits(np.concatenate(seg_ref)))
    # the one-launch entry, its own copy of the interval / rank / reduction code
    seg2, corr2, seg1, corr1 = _c_entries(vids, lens, packed)
    assert np.array_equal(_bits(seg2), _bits(seg_dev)) and np.array_equal(_bits(corr2), _bits(got[0]))
    assert np.array_equal(_bits(seg1), _bits(seg2))
    assert np.array_equal(np.isnan(corr1), np.isnan(corr2))
    np.testing.assert_allclose(corr1, corr2, rtol=0, atol=1e-12)
    _check_against_oracle("sumk_eval_device", corr1, want[0], corr_ref)


def test_one_launch_entry_on_the_plain_batch():
    """sumk_eval_device on the batch of test_device_tail_equals_host_tail: segment means bit-equal to sumk_eval_device_segments,
    correlations within 1e-12 of sumk_eval_device_spearman and of the host tail, and within the oracle gate."""
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    batch = []
    for i, (T, U) in enumerate([(300, 15), (1, 3), (97, 20), (650, 18), (33, 5), (320, 32), (150, 1)]):
        v = R.synthetic_video(T, 8100 + i, n_users=U)
        s = rng.random(T).astype(np.float32)
        if i == 2:
            s[10:40] = s[10]
        if i == 4:
            s[:] = 0.25
        batch.append((f"plain{i}", dict(v, n_steps=T), s))
    vids = [_prepare(v) for _, v, _ in batch]
    scores, lens = [s for _, _, s in batch], [T for _, v, _ in batch for T in [v["n_steps"]]]
    packed = torch.from_numpy(np.concatenate(scores)).to(dev)
    want = eval_native.evaluate_batch(vids, scores, 0.15, "knapsack", n_threads=3)
    seg2, corr2, seg1, corr1 = _c_entries(vids, lens, packed)
    corr_ref, seg_ref = _oracle(batch)
    assert np.array_equal(_bits(seg1), _bits(seg2)) and np.array_equal(_bits(seg2), _bits(np.concatenate(seg_ref)))
    assert np.array_equal(np.isnan(corr1), np.isnan(corr2))
    np.testing.assert_allclose(corr1, corr2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(corr1, want[0], rtol=0, atol=1e-12)
    assert _check_against_oracle("sumk_eval_device (plain batch)", corr1, want[0], corr_ref) == 2          # the one-step video and the all-tied one: constant frame scores
    _check_against_oracle("sumk_eval_device_spearman (plain batch)", corr2, want[0], corr_ref)


def test_scores_two_short_of_the_intervals_are_refused_and_not_cached():
    """lens[i] two or more short of the interval count is defined by nobody (the reference's loop raises IndexError)."""
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    v = R.synthetic_video(40, 8250, n_users=2)
    ok, short = _prepare(R.synthetic_video(20, 8251, n_users=2)), _prepare(v)
    lens = [20, 38]                                                          # 40 picks + sentinel = 40 intervals for 38 scores
    scores = [np.linspace(0, 1, T, dtype=np.float32) for T in lens]
    with pytest.raises(_lib.SumkError, match="more pick intervals than scores"):
        eval_native.evaluate_batch([ok, short], scores, 0.15, "knapsack")
    n_cached = len(eval_native._DEV_BATCH_CACHE)
    with pytest.raises(_lib.SumkError, match="40 pick intervals for 38 scores"):
        eval_native.evaluate_batch_device([ok, short], torch.from_numpy(np.concatenate(scores)).to(dev), lens, 0.15, "knapsack")
    assert _cache_entry([ok, short], lens, dev) is None and len(eval_native._DEV_BATCH_CACHE) == n_cached
    # one short is the defined case (the last interval takes 0), on both tails
    lens = [20, 39]
    scores = [np.linspace(0, 1, T, dtype=np.float32) for T in lens]
    want = eval_native.evaluate_batch([ok, short], scores, 0.15, "knapsack")
    got = eval_native.evaluate_batch_device([ok, short], torch.from_numpy(np.concatenate(scores)).to(dev), lens, 0.15, "knapsack")
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got[1], want[1])


def test_over_limit_descriptors_give_nan_and_leave_their_neighbours_alone():
    """A descriptor past the kernels' fixed LDS tables (4097 intervals; 33 annotators), which the Python wrapper refuses, handed straight to
    the three C entries: NaN for that video, the neighbouring videos' results unchanged.  Every pointer of every descriptor is a valid
    device allocation of the size the descriptor states: the guard is there so that nothing is written out of bounds, and nothing is."""
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(21)
    good = [R.synthetic_video(T, 8260 + i, n_users=U) for i, (T, U) in enumerate([(120, 3), (60, 32), (200, 7)])]
    many = R.edge_video(dict(n_frames=1, picks=np.zeros(4098, np.int32), change_points=np.array([[0, 0]], np.int32),
                             user_summary=np.zeros((2, 1), np.float32), n_steps=4098), "pick_spacing_2")
    assert len(many["picks"]) == 4098 and many["picks"][-1] != many["n_frames"]                       # 4097 intervals + the sentinel's: n_int = 4098
    crowd = R.synthetic_video(50, 8270, n_users=33)
    order = [good[0], many, good[1], crowd, good[2]]
    vids = [_prepare(v) for v in order]
    assert not eval_native.device_ready(vids[1]) and not eval_native.device_ready(vids[3])           # the wrapper refuses both
    lens = [len(v["picks"]) for v in order]
    scores = [rng.random(T).astype(np.float32) for T in lens]
    packed = torch.from_numpy(np.concatenate(scores)).to(dev)
    seg2, corr2, seg1, corr1 = _c_entries(vids, lens, packed)
    gi = [0, 2, 4]
    gseg2, gcorr2, gseg1, gcorr1 = _c_entries([vids[i] for i in gi], [lens[i] for i in gi], torch.from_numpy(np.concatenate([scores[i] for i in gi])).to(dev))
    seg_at = np.concatenate([[0], np.cumsum([v["cps"].shape[0] for v in vids])])
    sl = lambda a, i: a[seg_at[i]:seg_at[i + 1]]
    for seg, corr, gseg, gcorr in ((seg2, corr2, gseg2, gcorr2), (seg1, corr1, gseg1, gcorr1)):
        assert np.array_equal(_bits(np.concatenate([sl(seg, i) for i in gi])), _bits(gseg))
        assert np.array_equal(_bits(corr[gi]), _bits(gcorr)) and np.isfinite(gcorr).all()
        assert np.isnan(sl(seg, 1)).all() and np.isnan(corr[1]) and np.isnan(corr[3])
    # 33 annotators: the segment means do not involve them -- the two-launch form still delivers them, the one-launch kernel gives the video up whole
    alone = _c_entries([vids[3]], [lens[3]], torch.from_numpy(scores[3]).to(dev), override={0: dict(n_users=32)})[0]
    assert np.array_equal(_bits(sl(seg2, 3)), _bits(alone)) and np.isfinite(alone).all()
    assert np.isnan(sl(seg1, 3)).all()
