"""Kendall's tau-b on the device-side evaluation tail (csrc/evalkendall.hip: `evaluate_batch_device(metric="kendalltau")`) against the native
host tail (`evaluate_batch(metric="kendalltau")`, which tests/test_host_kendall.py holds to scipy and to an O(n^2) pair count on the CPU).

Both sides end in the same integer pair counts and the same three float64 operations (kendall_tau_b, csrc/evaldev_common.h), so the device
must give the host's counts with == and its correlations bit for bit.  Against scipy the tolerance is the one test_host_kendall.py derives
(three roundings per annotator and a mean over at most 32 values of magnitude <= 1: rtol 1e-13, atol 1e-14)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import recipes as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-13, 1e-14
METHODS = ["knapsack", "rank"]


def _prepare(v):
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    return eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"],
                                     E.rank_users(v["user_scores"]))


def _scipy(v, s):
    from summarizer_amd.utils import eval as E
    fs = E.upsample(np.atleast_1d(s), v["n_frames"], v["picks"])
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(E.evaluate_scores(fs, v["user_scores"], metric="kendalltau"))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_result(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:3], b[:3]))


class _Batch:
    """A batch with everything the tests share computed once: prepared videos, scores, the scipy values and the host tail's results."""
    def __init__(self, videos, scores, lens):
        from summarizer_amd.utils import eval_native
        self.scores, self.lens = scores, lens
        self.vids = [_prepare(v) for v in videos]
        self.scipy = np.array([_scipy(v, s) for v, s in zip(videos, scores)])
        self.host, self.spearman, self.host_counts = {}, {}, []
        for method in METHODS:
            self.host_counts = []
            self.host[method] = eval_native.evaluate_batch(self.vids, scores, 0.15, method, n_threads=3, metric="kendalltau", counts_out=self.host_counts)[:3]
            self.spearman[method] = eval_native.evaluate_batch(self.vids, scores, 0.15, method, n_threads=3)[:3]

    def subset(self, keep):
        sub = _Batch.__new__(_Batch)
        sub.vids, sub.scores, sub.lens = [self.vids[i] for i in keep], [self.scores[i] for i in keep], [self.lens[i] for i in keep]
        sub.scipy, sub.host_counts = self.scipy[keep], [self.host_counts[i] for i in keep]
        sub.host = {m: tuple(a[keep] for a in self.host[m]) for m in METHODS}
        sub.spearman = {m: tuple(a[keep] for a in self.spearman[m]) for m in METHODS}
        return sub

    def packed(self, dev):
        return torch.from_numpy(np.concatenate([np.atleast_1d(s) for s in self.scores])).to(dev)


@pytest.fixture(scope="module")
def tvsum():
    """The 50-video S-TVSum-shaped batch: T ~ U(150, 320), 20 annotators, ~3 500 frames each."""
    lens = [int(np.ceil(t)) for t in np.random.default_rng(0).uniform(150, 320, 50)]
    rng = np.random.default_rng(31)
    return _Batch([R.synthetic_video(T, 9800 + i, n_users=20) for i, T in enumerate(lens)], [rng.random(T).astype(np.float32) for T in lens], lens)


@pytest.fixture(scope="module")
def edges():
    """The geometries of recipes.eval_edge_batch (frames in front of the first pick tying with zero scores, picks[-1] == n_frames, repeated
    picks, one interval more than scores, 4000 / 4095 / 4096 intervals, 1 / 5 / 9 frames, -0.0; 1, 2, 31 and 32 annotators)."""
    batch = R.eval_edge_batch()
    return _Batch([v for _, v, _ in batch], [s for _, _, s in batch], [v["n_steps"] for _, v, _ in batch])


def _check_device(b, method):
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    assert all(eval_native.kendall_device_ready(v) for v in b.vids)
    packed, counts = b.packed(dev), []
    got = eval_native.evaluate_batch_device(b.vids, packed, b.lens, 0.15, method, n_threads=3, metric="kendalltau", counts_out=counts)
    want = b.host[method]
    for i, (c, h) in enumerate(zip(counts, b.host_counts)):
        assert np.array_equal(c, h), (i, c, h)
    assert _same_result(got, want), (got[0], want[0])                          # tau from the same integers, F-scores from the same segment means
    assert np.array_equal(np.isnan(got[0]), np.isnan(b.scipy))
    np.testing.assert_allclose(got[0], b.scipy, rtol=RTOL, atol=ATOL)
    assert np.array_equal(_bits(got[1]), _bits(b.spearman[method][1])) and np.array_equal(_bits(got[2]), _bits(b.spearman[method][2]))      # the metric does not reach the F-scores
    # again, and again with every cached device buffer of the batch filled with 0xFF bytes: the same bits
    again = eval_native.evaluate_batch_device(b.vids, packed, b.lens, 0.15, method, n_threads=3, metric="kendalltau")
    assert _same_result(again, got)
    ent = eval_native._DEV_BATCH_CACHE[(tuple(id(v) for v in b.vids), tuple(int(T) for T in b.lens), str(dev))]
    for t in (ent["buffers"]["scratch"], ent["buffers"]["seg"], ent["buffers"]["corr"], ent["kendall"]["buffers"]["tau"], ent["kendall"]["buffers"]["counts"]):
        t.view(torch.uint8).fill_(255)
    counts3 = []
    third = eval_native.evaluate_batch_device(b.vids, packed, b.lens, 0.15, method, n_threads=3, metric="kendalltau", counts_out=counts3)
    assert _same_result(third, got) and all(np.array_equal(c, h) for c, h in zip(counts3, counts))
    return got


@pytest.mark.parametrize("method", METHODS)
def test_device_equals_host_on_the_tvsum_batch(tvsum, method):
    got = _check_device(tvsum, method)
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() < 1


@pytest.mark.parametrize("method", METHODS)
def test_device_equals_host_on_the_edge_batch(edges, method):
    got = _check_device(edges, method)
    assert int(np.isnan(got[0]).sum()) == 2                                    # n_frames_1 and all_zero+picks_from_7: constant frame scores


def test_spearman_is_untouched_by_kendall_calls_on_the_same_batch(edges):
    """One cache entry serves both metrics: Spearman before, Kendall, Spearman after -- the Spearman results are the same bits."""
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    packed = edges.packed(dev)
    before = eval_native.evaluate_batch_device(edges.vids, packed, edges.lens, 0.15, "knapsack", n_threads=3)
    kendall = eval_native.evaluate_batch_device(edges.vids, packed, edges.lens, 0.15, "knapsack", n_threads=3, metric="kendalltau")
    after = eval_native.evaluate_batch_device(edges.vids, packed, edges.lens, 0.15, "knapsack", n_threads=3, metric="spearmanr")
    assert _same_result(before, after) and not _same_result(before, kendall)
    assert np.array_equal(_bits(kendall[1]), _bits(before[1])) and np.array_equal(_bits(kendall[2]), _bits(before[2]))
    np.testing.assert_allclose(before[0], edges.spearman["knapsack"][0], rtol=0, atol=1e-12)
    with pytest.raises(KeyError, match="Unknown metric pearson"):
        eval_native.evaluate_batch_device(edges.vids, packed, edges.lens, 0.15, "knapsack", metric="pearson")


# ------------------------------------------------------------------------------------------------ the LDS bound
def _long_video(n_frames, seed, n_users=2):
    """A video of exactly n_frames frames, picks every 15th, annotator scores distinct per frame (no run of the sort is trivial)."""
    rng = np.random.default_rng(seed)
    T = (n_frames + 14) // 15
    cuts = np.sort(rng.choice(np.arange(15, n_frames - 15), size=7, replace=False))
    starts, ends = np.concatenate([[0], cuts]), np.concatenate([cuts - 1, [n_frames - 1]])
    us = rng.random((n_users, n_frames)).astype(np.float32)
    us[1, ::3] = us[1, 0]                                                      # and one annotator with a large tie group
    return dict(n_frames=n_frames, picks=(15 * np.arange(T)).astype(np.int32), change_points=np.stack([starts, ends], axis=1).astype(np.int32),
                n_frame_per_seg=(ends - starts + 1).astype(np.int32), user_summary=(rng.random((n_users, n_frames)) < 0.15).astype(np.float32),
                user_scores=us, n_steps=T)


@pytest.fixture(scope="module")
def bound():
    from summarizer_amd.utils import eval_native
    M = eval_native.KENDALL_MAX_FRAMES
    assert M == 16384
    videos = [_long_video(M, 9900), _long_video(M - 1, 9901), _long_video(M + 1, 9902), R.synthetic_video(40, 9903, n_users=3)]
    rng = np.random.default_rng(32)
    lens = [v.get("n_steps", len(v["picks"])) for v in videos]
    return _Batch(videos, [rng.random(T).astype(np.float32) for T in lens], lens)


def test_videos_at_the_lds_bound_run_on_the_device_and_one_above_it_is_declined(bound):
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    ready = [eval_native.kendall_device_ready(v) for v in bound.vids]
    assert ready == [True, True, False, True] and all(eval_native.device_ready(v) for v in bound.vids)
    np.testing.assert_allclose(bound.host["knapsack"][0], bound.scipy, rtol=RTOL, atol=ATOL)          # the host path serves the long one
    with pytest.raises(_lib.SumkError, match="16385 frames"):
        eval_native.evaluate_batch_device(bound.vids, bound.packed(dev), bound.lens, 0.15, "knapsack", metric="kendalltau")
    eval_native.evaluate_batch_device(bound.vids, bound.packed(dev), bound.lens, 0.15, "knapsack")   # (Spearman takes all four)
    sub = bound.subset([0, 1, 3])
    got = _check_device(sub, "knapsack")
    assert np.isfinite(got[0]).all()


def _kendall_c_entry(vids, lens, scores_dev, override=None):
    """sumk_eval_device_kendall on descriptors and 0xFF-filled buffers of the test's own.  override: {video: {descriptor field: value}}."""
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    lib = _lib.load()
    dev, n = scores_dev.device, len(vids)
    descr, kd = (_lib.EvalDevVideo * n)(), (_lib.EvalDevKendall * n)()
    keep, row0, frame0, seg0, users = [], 0, 0, 0, 0
    for i, (v, T) in enumerate(zip(vids, lens)):
        m = eval_native._device_meta(v, dev, kendall=True); keep.append(m)
        assert m["ydense"].shape == v["user_ranks"].shape and m["ydense"].dtype == torch.int32 and m["ytie"].dtype == torch.int64
        e = descr[i]
        e.picks, e.n_picks, e.n_frames, e.n_steps = m["picks"].data_ptr(), v["picks"].shape[0], v["n_frames"], int(T)
        e.row0, e.frame0 = row0, frame0
        e.cps, e.n_segs, e.seg0 = m["cps"].data_ptr(), v["cps"].shape[0], seg0
        e.user_ranks, e.user_mean, e.user_ssq, e.n_users = m["ranks"].data_ptr(), m["mean"].data_ptr(), m["ssq"].data_ptr(), v["user_ranks"].shape[0]
        kd[i].y_dense, kd[i].ytie, kd[i].counts0 = m["ydense"].data_ptr(), m["ytie"].data_ptr(), users
        for k, val in (override or {}).get(i, {}).items():
            setattr(e, k, val)
        row0 += int(T); frame0 += v["n_frames"]; seg0 += v["cps"].shape[0]; users += v["user_ranks"].shape[0]
    assert row0 <= scores_dev.numel()
    up = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).to(dev)
    descr_dev, kd_dev = up(descr), up(kd)

    def poisoned(numel, dtype):
        t = torch.empty(numel, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(255)
        return t
    tau = poisoned(lib.sumk_eval_device_kendall_scratch_bytes(n, frame0) // 8, torch.float64)
    corr, counts = poisoned(n, torch.float64), poisoned(4 * users, torch.int64)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.sumk_eval_device_kendall(scores_dev.data_ptr(), descr_dev.data_ptr(), kd_dev.data_ptr(), n, tau.data_ptr(), corr.data_ptr(),
                                            counts.data_ptr(), st), "sumk_eval_device_kendall")
    torch.cuda.synchronize(dev)
    per_video = np.cumsum([v["user_ranks"].shape[0] for v in vids])[:-1]
    return corr.cpu().numpy(), np.split(counts.cpu().numpy().reshape(-1, 4), per_video)


def test_over_limit_descriptors_give_nan_and_leave_their_neighbours_alone(bound):
    """Descriptors the Python wrapper declines -- 16 385 frames, 4 098 pick intervals, 33 annotators -- handed straight to the C entry between
    good ones.  Every pointer is a valid allocation of the size its descriptor states: the guards are there so that nothing is written out of
    bounds, and the neighbours' bits show that nothing was."""
    from summarizer_amd.utils import eval_native
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(33)
    good = [_prepare(R.synthetic_video(T, 9910 + i, n_users=U)) for i, (T, U) in enumerate([(120, 3), (60, 32), (200, 7)])]
    many = _prepare(R.edge_video(dict(n_frames=1, picks=np.zeros(4098, np.int32), change_points=np.array([[0, 0]], np.int32),
                                      user_summary=np.zeros((2, 1), np.float32), n_steps=4098), "pick_spacing_2"))
    crowd = _prepare(R.synthetic_video(50, 9920, n_users=33))
    long_ = bound.vids[2]
    assert long_["n_frames"] == eval_native.KENDALL_MAX_FRAMES + 1
    vids = [good[0], long_, good[1], many, crowd, good[2]]
    assert [eval_native.kendall_device_ready(v) for v in vids] == [True, False, True, False, False, True]
    lens = [len(v["picks"]) for v in vids]
    scores = [rng.random(T).astype(np.float32) for T in lens]
    corr, counts = _kendall_c_entry(vids, lens, torch.from_numpy(np.concatenate(scores)).to(dev))
    gi = [0, 2, 5]
    gcorr, gcounts = _kendall_c_entry([vids[i] for i in gi], [lens[i] for i in gi], torch.from_numpy(np.concatenate([scores[i] for i in gi])).to(dev))
    assert np.array_equal(_bits(corr[gi]), _bits(gcorr)) and np.isfinite(gcorr).all()
    for i, g in zip(gi, gcounts):
        assert np.array_equal(counts[i], g)
    want = eval_native.evaluate_batch([vids[i] for i in gi], [scores[i] for i in gi], metric="kendalltau")[0]
    assert np.array_equal(_bits(gcorr), _bits(want))
    assert np.isnan(corr[[1, 3, 4]]).all()
    assert (counts[1] == -1).all() and (counts[3] == -1).all() and (counts[4] == -1).all()      # (33 annotators: never written, the fill's -1)


# ------------------------------------------------------------------------------------------------ Trainer.test
def _trainer(ds, keys, **over):
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.hps import make_hps
    hps = make_hps(ds, [{"train_keys": [], "test_keys": keys}], epochs=1, extra_params={"input_size": "128"}, **over)
    torch.manual_seed(77)
    return VASNetTrainer(hps, hps.splits_files[0]).reset()


def _scipy_trainer_path(tr, keys):
    """Trainer._eval_scores (scipy, one annotator and one video at a time) on the scores of the packed launch Trainer.test itself makes."""
    tr.model.eval()
    with torch.no_grad():
        return tr._eval_scores(tr._score_keys(keys), keys)


def test_trainer_test_with_kendall():
    from summarizer_amd.utils import eval_native
    from summarizer_amd.utils.datasets import DictDataset, synthetic_dataset
    ds = synthetic_dataset(6, seed=41, D=128, t_range=(30, 90), n_users=5)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
    tr = _trainer(ds, keys)
    assert tr._correlation_metric() == "spearmanr"
    before = tr.test(0)
    tr.hps.correlation_metric = "kendalltau"
    n_entries = len(eval_native._DEV_BATCH_CACHE)
    kendall = tr.test(0)
    assert len(eval_native._DEV_BATCH_CACHE) == n_entries                      # the device tail ran, on the Spearman run's cache entry
    assert "kendall" in eval_native._DEV_BATCH_CACHE[next(reversed(eval_native._DEV_BATCH_CACHE))]
    np.testing.assert_allclose(kendall[0], _scipy_trainer_path(tr, keys), rtol=RTOL, atol=ATOL)
    assert kendall[1] == before[1] and kendall[0] != before[0]                 # F-scores: the same bits under either metric
    assert tr.test(0) == kendall                                               # repeatable
    tr.hps.correlation_metric = "spearmanr"
    assert tr.test(0) == before                                                # no cross-talk through the shared cache entry
    # one video stops qualifying for the device tail: the whole batch takes the native host tail, with the same numbers
    tr.hps.correlation_metric = "kendalltau"
    tr._native_meta(keys[2])["_dev_ready"] = False
    assert tr._test_on_device(keys) is None
    assert tr.test(0) == kendall
    tr.hps.correlation_metric = "pearson"
    with pytest.raises(KeyError, match="Unknown metric pearson"):
        tr.test(0)
    # a video past the Kendall kernel's frame bound: Spearman still runs on the device, Kendall declines to the host threads
    long_ds = synthetic_dataset(1, seed=42, D=128, t_range=(1100, 1100.5), n_users=3)
    both = DictDataset({**{k: {f: ds[k][f][...] for f in ds[k]} for k in keys[:2]}, "video_9": {f: long_ds["video_1"][f][...] for f in long_ds["video_1"]}})
    keys2 = keys[:2] + ["video_9"]
    assert int(both["video_9"]["n_frames"][()]) > eval_native.KENDALL_MAX_FRAMES
    tr2 = _trainer(both, keys2)
    spearman2 = tr2.test(0)
    assert tr2._test_on_device(keys2) is not None
    tr2.hps.correlation_metric = "kendalltau"
    assert tr2._test_on_device(keys2) is None
    kendall2 = tr2.test(0)
    np.testing.assert_allclose(kendall2[0], _scipy_trainer_path(tr2, keys2), rtol=RTOL, atol=ATOL)
    assert kendall2[1] == spearman2[1]
