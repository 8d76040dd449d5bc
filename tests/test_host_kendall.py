"""CPU: Kendall's tau-b of the native host tail (`evaluate_batch(metric="kendalltau")` -> sumk_eval_videos_kendall, csrc/evaltail.hip) against
scipy (`eval.evaluate_scores(metric="kendalltau")`, the specification) and against an O(n^2) sign-matrix count of the pairs.

Tolerance against scipy, derived: the pair counts are integers and exact on both sides, so the two differ by the three float64 roundings
per annotator (a division, two square roots and a division: a few ulp of a value of magnitude <= 1) and a mean over at most 32 such values
-- rtol 1e-13, atol 1e-14 is a hundred times that.  The counts themselves are compared with ==, and tau recomputed from them bit for bit."""
import warnings

import numpy as np
import pytest

import recipes as R

RTOL, ATOL = 1e-13, 1e-14


def _prep(v):
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    return eval_native.prepare_video(v["n_frames"], v["picks"], v.get("change_points"), v.get("n_frame_per_seg"), v.get("user_summary"),
                                     E.rank_users(v["user_scores"]))


def _scipy(v, s):
    from summarizer_amd.utils import eval as E
    fs = E.upsample(np.atleast_1d(s), v["n_frames"], v["picks"])
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(E.evaluate_scores(fs, v["user_scores"], metric="kendalltau"))


def _native(videos, scores, **kw):
    from summarizer_amd.utils import eval_native
    counts = []
    corr = eval_native.evaluate_batch([_prep(v) for v in videos], scores, metric="kendalltau", counts_out=counts, **kw)[0]
    return corr, counts


def _brute_counts(x, user_scores):
    """{cmd, xtie, ytie, ntie} per annotator from the n x n sign matrices of the frame scores and the annotator's scores themselves
    (every pair twice, the diagonal tied)."""
    n = x.shape[0]
    sx = (x[:, None] > x[None, :]).astype(np.int8) - (x[:, None] < x[None, :]).astype(np.int8)
    out = []
    for y in user_scores:
        sy = (y[:, None] > y[None, :]).astype(np.int8) - (y[:, None] < y[None, :]).astype(np.int8)
        cmd = int((sx * sy).sum(dtype=np.int64)) // 2
        xtie = (int((sx == 0).sum()) - n) // 2
        ytie = (int((sy == 0).sum()) - n) // 2
        ntie = (int(((sx == 0) & (sy == 0)).sum()) - n) // 2
        out.append([cmd, xtie, ytie, ntie])
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def _tau_from_counts(c, n):
    """scipy's three operations on the integer counts, then np.mean over the annotators."""
    tot = n * (n - 1) // 2
    taus = []
    for cmd, xtie, ytie, _ in c.tolist():
        if xtie == tot or ytie == tot:
            taus.append(np.nan)
        else:
            taus.append(float(np.minimum(1., max(-1., cmd / np.sqrt(tot - xtie) / np.sqrt(tot - ytie)))))
    return float(np.mean(taus))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _check_against_scipy(videos, scores, **kw):
    got, _ = _native(videos, scores, **kw)
    want = np.array([_scipy(v, s) for v, s in zip(videos, scores)])
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    return got, want


def _check_against_brute(videos, scores):
    from summarizer_amd.utils import eval as E
    got, counts = _native(videos, scores)
    assert len(counts) == len(videos)
    for i, (v, s) in enumerate(zip(videos, scores)):
        assert v["n_frames"] <= 3000
        fs = E.upsample(np.atleast_1d(s), v["n_frames"], v["picks"])
        want = _brute_counts(fs, v["user_scores"])
        assert counts[i].dtype == np.int64 and np.array_equal(counts[i], want), (i, counts[i], want)
        assert _same_bits(got[i], _tau_from_counts(counts[i], v["n_frames"])), (i, got[i], _tau_from_counts(counts[i], v["n_frames"]))
    return got, counts


@pytest.mark.parametrize("T", [120, 300, 640])
def test_single_video_against_scipy(T):
    v = R.synthetic_video(T, 9100 + T, n_users=15)
    s = np.random.default_rng(T).random(T).astype(np.float32)
    got, _ = _check_against_scipy([v], [s])
    assert np.isfinite(got).all() and abs(got[0]) < 1


def test_ragged_batch_against_scipy_on_every_thread_path():
    rng = np.random.default_rng(5)
    shapes = [(1, 3), (33, 5), (97, 20), (150, 1), (200, 32), (64, 2), (15, 7), (301, 15), (250, 18), (2, 4)]
    videos = [R.synthetic_video(T, 9200 + i, n_users=U) for i, (T, U) in enumerate(shapes)]
    scores = [rng.random(T).astype(np.float32) for T, _ in shapes]
    scores[2][10:40] = scores[2][10]                      # equal step scores: tie groups across pick intervals
    pool, _ = _check_against_scipy(videos, scores)         # the persistent pool
    assert np.isnan(pool[0]) and np.isfinite(pool[1:]).all()          # one step: constant frame scores
    one, _ = _check_against_scipy(videos, scores, n_threads=1)
    three, _ = _check_against_scipy(videos, scores, n_threads=3)
    assert _same_bits(pool, one) and _same_bits(pool, three)


def test_counts_equal_the_pair_count_and_tau_follows_from_them_bit_for_bit():
    rng = np.random.default_rng(6)
    shapes = [(200, 3), (97, 2), (31, 4), (2, 2)]
    videos = [R.synthetic_video(T, 9300 + i, n_users=U) for i, (T, U) in enumerate(shapes)]
    scores = [rng.random(T).astype(np.float32) for T, _ in shapes]
    scores[0][50:90] = scores[0][3]
    got, counts = _check_against_brute(videos, scores)
    assert [c.shape for c in counts] == [(U, 4) for _, U in shapes]
    assert (counts[0][:, 1] > 0).all() and (counts[0][:, 3] > 0).all()          # ties on the machine side, and joint ones
    _check_against_scipy(videos, scores)


def _edge(name, T, U, seed, kind):
    v = dict(R.synthetic_video(T, seed, n_users=U), n_steps=T)
    v = R.edge_video(v, name)
    return v, R.edge_scores(kind, v["n_steps"], seed + 1)


def test_heavy_ties_and_constant_vectors():
    rng = np.random.default_rng(7)
    five = R.synthetic_video(120, 9400, n_users=4)
    five["user_scores"] = (rng.integers(0, 5, size=five["user_scores"].shape) / 4).astype(np.float32)      # five levels
    s5 = rng.random(120).astype(np.float32)
    const_user = R.synthetic_video(80, 9401, n_users=3)
    const_user["user_scores"][1, :] = 0.5                                                                  # one constant annotator
    const_machine = R.synthetic_video(60, 9402, n_users=3)
    videos, scores = [five, const_user, const_machine], [s5, rng.random(80).astype(np.float32), np.full(60, 0.25, np.float32)]
    got, counts = _check_against_brute(videos, scores)
    _check_against_scipy(videos, scores)
    assert np.isfinite(got[0]) and np.isnan(got[1]) and np.isnan(got[2])
    n = const_user["n_frames"]
    assert counts[1][1, 2] == n * (n - 1) // 2 and counts[1][0, 2] < n * (n - 1) // 2       # ytie == tot for the constant annotator alone
    n = const_machine["n_frames"]
    assert (counts[2][:, 1] == n * (n - 1) // 2).all()                                      # xtie == tot


def test_uncovered_frames_tie_with_zero_scores_and_last_pick_at_the_end():
    from summarizer_amd.utils import eval as E
    front, s_front = _edge("picks_from_7", 45, 2, 9500, "zeros")
    assert front["picks"][0] == 7 and (s_front == 0).sum() >= 10
    neg, s_neg = _edge("picks_from_15", 60, 3, 9501, "negative")                    # -0.0, +0.0 and the uncovered frames: one tie group
    assert np.signbit(s_neg[s_neg == 0]).any() and not np.signbit(s_neg[s_neg == 0]).all()
    last, s_last = _edge("last_pick_is_n_frames", 80, 3, 9502, "random")
    assert last["picks"][-1] == last["n_frames"]
    more, s_more = _edge("one_more_interval", 40, 2, 9503, "random")
    videos, scores = [front, neg, last, more], [s_front, s_neg, s_last, s_more]
    got, counts = _check_against_brute(videos, scores)
    _check_against_scipy(videos, scores)
    assert np.isfinite(got).all()
    # the zero tie group of `front`: the 7 uncovered frames and every frame of a zero-score interval are ONE group
    fs = E.upsample(s_front, front["n_frames"], front["picks"])
    z = int((fs == 0).sum())
    assert z > 7 and counts[0][0, 1] >= z * (z - 1) // 2


def test_two_frames_one_frame():
    two = dict(n_frames=2, picks=np.array([0, 1], np.int32), user_scores=np.array([[0.2, 0.7], [0.9, 0.1], [0.3, 0.3]], np.float32))
    one = dict(n_frames=1, picks=np.array([0], np.int32), user_scores=np.array([[0.2], [0.9]], np.float32))
    pair = dict(two, user_scores=two["user_scores"][:2])
    s2 = np.array([0.1, 0.9], np.float32)
    got, counts = _native([two, one, pair], [s2, np.array([0.5], np.float32), s2])
    assert np.array_equal(counts[2], [[1, 0, 0, 0], [-1, 0, 0, 0]]) and got[2] == 0.0        # tau = +1 and -1
    assert np.array_equal(counts[0][2], [0, 0, 1, 0]) and np.isnan(got[0])                   # a tied annotator: NaN, and so the video's mean
    assert np.isnan(got[1]) and np.array_equal(counts[1], [[0, 0, 0, 0], [0, 0, 0, 0]])      # one frame: no pairs
    _check_against_scipy([two, one, pair], [s2, np.array([0.5], np.float32), s2])


def test_perfectly_concordant_and_discordant():
    """50 frames of distinct scores: tot = 1225 = 35^2, so tot / sqrt(tot) / sqrt(tot) has no rounding and the result is exactly +-1 (with
    another count the three operations may land one ulp below 1, in scipy as here: the tied video is held to the formula instead)."""
    from summarizer_amd.utils import eval as E
    rng = np.random.default_rng(8)
    n = 50
    s = rng.permutation(n).astype(np.float32) / n
    up = dict(n_frames=n, picks=np.arange(n, dtype=np.int32), user_scores=np.stack([s, 2 * s + 1]).astype(np.float32))
    down = dict(up, user_scores=np.stack([-s, 1 - s]).astype(np.float32))
    got, counts = _native([up, down], [s, s])
    assert got[0] == 1.0 and got[1] == -1.0
    assert np.array_equal(counts[0], [[1225, 0, 0, 0]] * 2) and np.array_equal(counts[1], [[-1225, 0, 0, 0]] * 2)
    # piecewise-constant scores against themselves: every pair concordant or jointly tied
    v = R.synthetic_video(40, 9600, n_users=2)
    sv = rng.random(40).astype(np.float32)
    fs = E.upsample(sv, v["n_frames"], v["picks"])
    v["user_scores"] = np.stack([fs, -fs])
    got, counts = _check_against_brute([v], [sv])
    tot = v["n_frames"] * (v["n_frames"] - 1) // 2
    assert counts[0][0, 0] == tot - counts[0][0, 1] and counts[0][1, 0] == -(tot - counts[0][1, 1])
    assert (counts[0][:, 1] == counts[0][:, 2]).all() and (counts[0][:, 1] == counts[0][:, 3]).all()
    assert abs(got[0]) < 1e-15                                                              # (+1 - 1) / 2 up to the last place
    _check_against_scipy([v], [sv])


def test_metric_keyword():
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    v = R.synthetic_video(90, 9700, n_users=6)
    s = np.random.default_rng(9).random(90).astype(np.float32)
    p = _prep(v)
    with pytest.raises(KeyError, match="Unknown metric pearson"):
        eval_native.evaluate_batch([p], [s], metric="pearson")
    with pytest.raises(KeyError, match="Unknown metric pearson"):
        eval_native.evaluate_batch_device([p], None, [90], metric="pearson")
    fs = E.upsample(s, v["n_frames"], v["picks"])
    default = eval_native.evaluate_batch([p], [s])
    named = eval_native.evaluate_batch([p], [s], metric="spearmanr")
    assert all(_same_bits(a, b) for a, b in zip(default[:3], named[:3]))
    np.testing.assert_allclose(default[0][0], E.evaluate_scores(fs, v["user_scores"]), rtol=0, atol=1e-12)
    kendall = eval_native.evaluate_batch([p], [s], metric="kendalltau")
    assert _same_bits(kendall[1], default[1]) and _same_bits(kendall[2], default[2])          # the F-scores do not depend on the metric
    assert kendall[0][0] != default[0][0]
    np.testing.assert_allclose(kendall[0][0], _scipy(v, s), rtol=RTOL, atol=ATOL)
