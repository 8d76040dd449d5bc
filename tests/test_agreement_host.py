"""CPU: the specification of the inter-annotator agreement (tests/agreement_ref.py) against the real-reference golden and against cases
small enough to compute by hand, and everything `summarizer_amd.utils.agreement` and the three C entries refuse on the host before they
touch the GPU.  F is exact (float32, operation for operation); the correlations are held to scipy at the gates of tests/test_host_eval.py
(Spearman: rtol 1e-12, atol 1e-15) and tests/test_host_kendall.py (Kendall: rtol 1e-13, atol 1e-14)."""
import ctypes as C

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import agreement_ref as R
from summarizer_amd import _lib
from summarizer_amd._lib import SumkError
from summarizer_amd.utils import agreement as M
from summarizer_amd.utils import eval as E

F32, F64 = np.float32, np.float64
GATES = {"spearmanr": dict(rtol=1e-12, atol=1e-15), "kendalltau": dict(rtol=1e-13, atol=1e-14)}


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


@pytest.fixture(scope="module")
def gold(golden):
    return golden("agreement")


# ------------------------------------------------------------------------------------------------ the specification against the golden
def test_golden_is_what_its_generator_promises(gold):
    us, sc = gold["user_summary"], gold["user_scores"]
    assert us.shape == sc.shape == (5, 611)
    on = us > 0
    assert all((on[a] & on[b]).any() for a in range(5) for b in range(5))
    assert all(np.unique(sc[u]).size > 1 for u in range(5))


def test_spec_f_equals_golden_exactly(gold):
    r = R.f_agreement(gold["user_summary"])
    assert r["F"].dtype == F32 and r["f_avg_user"].dtype == F32
    assert_array_equal(_bits(r["F"]), _bits(gold["F"]))
    assert_array_equal(_bits(r["f_avg_user"]), _bits(gold["f_avg_user"]))
    assert_array_equal(_bits(r["f_max_user"]), _bits(gold["f_max_user"]))
    assert r["f_avg"] == np.mean(gold["f_avg_user"].astype(F64)) and r["f_max"] == np.mean(gold["f_max_user"].astype(F64))
    # the package's own host tail computes the same pairs
    for a in range(5):
        others = [b for b in range(5) if b != a]
        avg, mx = E.evaluate_summary(gold["user_summary"][a], gold["user_summary"][others])
        assert avg == r["f_avg_user"][a] and mx == r["f_max_user"][a]


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_spec_correlations_equal_golden_within_the_scipy_gates(gold, metric):
    r = R.corr_agreement(gold["user_scores"], metric)
    np.testing.assert_allclose(r["C"], gold[f"{metric}/C"], **GATES[metric])
    np.testing.assert_allclose(r["corr_user"], gold[f"{metric}/corr_user"], **GATES[metric])
    np.testing.assert_allclose(r["corr"], np.mean(gold[f"{metric}/corr_user"]), **GATES[metric])
    print(f"AGREEMENT-HOST-REPORT {metric}: worst |spec - reference| = {np.abs(r['C'] - gold[f'{metric}/C']).max():.3e}")


def test_written_out_means_are_numpys():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 8, 9, 19, 31, 32):
        a = rng.random(n)
        assert R.mean64(a) == np.mean(a), n
    assert np.isnan(R.mean64(np.array([0.5, np.nan, 0.25])))


def test_kendall_counts_equal_the_pair_count():
    """The integer counts of the specification against the n x n sign matrices, on graded, continuous and equal rows."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 50, 257):
        x = np.stack([rng.integers(0, 5, n).astype(F32), rng.random(n).astype(F32), rng.integers(0, 3, n).astype(F32)])
        x = np.concatenate([x, x[1:2]])
        _, counts = R.kendall_matrix(x)
        for a in range(4):
            sx = np.sign(x[a][:, None] - x[a][None, :])
            for b in range(4):
                sy = np.sign(x[b][:, None] - x[b][None, :])
                want = (int((sx * sy).sum()) // 2, (int((sx == 0).sum()) - n) // 2, (int((sy == 0).sum()) - n) // 2,
                        (int(((sx == 0) & (sy == 0)).sum()) - n) // 2)
                assert tuple(counts[a, b]) == want, (n, a, b)


def test_rank_rows_spec_is_the_host_metadata():
    """What sumk_rank_rows is specified to leave = what eval.rank_users, eval_native._kendall_meta and _device_meta compute today."""
    from summarizer_amd.utils import eval_native
    x = np.stack([R.graded(1, 300, 1)[0], R.continuous(1, 300, 2)[0], np.full(300, 0.5, F32), np.where(np.arange(300) % 2, F32(-0.0), F32(0.0))])
    r = R.rank_rows(x)
    ru = E.rank_users(x)
    assert_array_equal(r["ranks"], ru)
    dense, ytie = eval_native._kendall_meta({"user_ranks": ru})
    assert_array_equal(r["dense"], dense); assert_array_equal(r["ties"], ytie)
    mu = ru.sum(axis=1) / ru.shape[1]
    assert_array_equal(r["mean"], mu); assert_array_equal(r["ssq"], ((ru - mu[:, None]) ** 2).sum(axis=1))
    assert r["ties"][2] == 300 * 299 // 2 and r["ties"][3] == 300 * 299 // 2 and r["dense"][3].max() == 0


# ------------------------------------------------------------------------------------------------ hand cases, from the specification alone
def test_identical_summaries_give_one():
    row = np.array([0, 2, 0, 1, 1, 0], F32)
    r = R.f_agreement(np.stack([row, row, row]))
    assert_array_equal(r["F"], np.ones((3, 3), F32))
    assert_array_equal(r["f_avg_user"], np.ones(3, F32)); assert r["f_avg"] == 1.0 and r["f_max"] == 1.0


def test_empty_and_disjoint_summaries_give_zero_in_float32():
    us = np.array([[1, 1, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0]], F32)
    r = R.f_agreement(us)
    want = np.zeros((3, 3), F32); want[0, 0] = want[1, 1] = 1
    assert_array_equal(r["F"], want)                                 # the empty row against itself: P = R = 0 -> 0
    assert r["f_avg_user"].dtype == F32 and r["f_max_user"].dtype == F32
    assert_array_equal(r["f_avg_user"], np.zeros(3, F32)); assert r["f_avg"] == 0.0 and isinstance(r["f_avg"], F64)


def test_f_by_hand():
    """o = 1, sums 2 and 1: P = 1/2, R = 1 (float32, the 1e-8 vanishes), F = 2 * .5 * 1 / 1.5."""
    r = R.f_agreement(np.array([[1, 1, 0], [1, 0, 0]], F32))
    f = F32(F32(F32(F32(2) * F32(0.5)) * F32(1)) / F32(1.5))
    assert_array_equal(r["F"], np.array([[1, f], [f, 1]], F32))
    assert_array_equal(r["f_avg_user"], np.array([f, f], F32)); assert_array_equal(r["f_max_user"], np.array([f, f], F32))
    assert r["f_avg"] == F64(f)


def test_one_annotator_is_nan():
    r = R.agreement(np.array([[1, 0, 1]], F32), np.array([[0.1, 0.2, 0.3]], F32))
    assert np.isnan(r["f_avg"]) and np.isnan(r["f_max"]) and np.isnan(r["corr"])
    assert np.isnan(r["f_avg_user"]).all() and np.isnan(r["corr_user"]).all() and r["F"][0, 0] == 1
    assert np.isnan(R.corr_agreement(np.array([[0.1, 0.2, 0.3]], F32), "kendalltau")["corr"])


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_constant_row_is_a_nan_row_and_column(metric):
    x = np.array([[1, 2, 3, 4, 5], [5, 5, 5, 5, 5], [2, 1, 4, 3, 5]], F32)
    r = R.corr_agreement(x, metric)
    assert np.isnan(r["C"][1]).all() and np.isnan(r["C"][:, 1]).all() and np.isfinite(r["C"][0, 2]) and np.isfinite(r["C"][2, 0])
    assert np.isnan(r["corr_user"]).all() and np.isnan(r["corr"])          # every leave-one-out mean meets the constant row
    np.testing.assert_allclose(r["C"], R.scipy_matrix(x, metric), **GATES[metric])


def test_tau_swaps_the_tie_counts():
    x = np.array([[1, 1, 2, 3, 3, 3, 4], [1, 2, 2, 3, 1, 5, 6]], F32)
    tau, counts = R.kendall_matrix(x)
    assert counts[0, 1, 0] == counts[1, 0, 0] and counts[0, 1, 3] == counts[1, 0, 3]
    assert counts[0, 1, 1] == counts[1, 0, 2] == 4 and counts[0, 1, 2] == counts[1, 0, 1] == 2
    tot = 21
    assert tau[0, 1] == R.kendall_tau_b(counts[0, 1, 0], tot, 4, 2) and tau[1, 0] == R.kendall_tau_b(counts[0, 1, 0], tot, 2, 4)
    np.testing.assert_allclose(tau, R.scipy_matrix(x, "kendalltau"), **GATES["kendalltau"])


def test_f_and_rho_are_bitwise_symmetric():
    F = R.f_matrix(R.selections(9, 611, 4))
    assert_array_equal(_bits(F), _bits(F.T.copy()))
    rho = R.spearman_matrix(np.concatenate([R.graded(4, 611, 5), R.continuous(4, 611, 6)]))
    assert_array_equal(_bits(rho), _bits(rho.T.copy()))


def test_equal_rows_correlate_perfectly():
    x = R.graded(3, 200, 8)
    x[2] = x[0]
    assert R.kendall_matrix(x)[0][0, 2] == 1.0
    assert abs(R.spearman_matrix(x)[0, 2] - 1.0) <= 2.3e-16


# ------------------------------------------------------------------------------------------------ the binding and the host-side refusals
def test_abi_of_the_new_entries():
    assert C.sizeof(_lib.AgreementVideo) == 72           # two pointers, four int32, five int64
    lib = _lib.load()
    for name in ("sumk_rank_rows", "sumk_agreement_f", "sumk_agreement_corr"):
        assert hasattr(lib, name) and name in _lib._SIGS
    assert M.MAX_USERS == 32 and M.MAX_RANK_FRAMES == 16384 and M.MAX_FRAMES == 1 << 24 and M.METRICS == {"spearmanr": 0, "kendalltau": 1}


def _video(n_frames=60, U=3, **over):
    v = {"user_summary": (np.arange(U * n_frames).reshape(U, n_frames) % 3 == 0).astype(F32),
         "user_scores": ((np.arange(U * n_frames).reshape(U, n_frames) * 7 % 5) / 4).astype(F32)}
    v.update(over)
    return {k: x for k, x in v.items() if x is not None}


REFUSALS = {
    "nothing to compare": (dict(user_summary=None, user_scores=None), "video bad has neither user_summary nor user_scores"),
    "summary 1-d": (dict(user_summary=np.ones(60, F32)), r"video bad: user_summary must be \(n_users, n_frames\)"),
    "scores 3-d": (dict(user_scores=np.ones((2, 3, 10), F32)), r"video bad: user_scores must be \(n_users, n_frames\)"),
    "scores not finite": (dict(user_scores=np.where(np.arange(180).reshape(3, 60) == 77, np.nan, 0.5).astype(F32)), "video bad: user_scores must be finite"),
    "summary not finite": (dict(user_summary=np.full((3, 60), np.inf, F32)), "video bad: user_summary must be finite"),
    "frames disagree": (dict(user_scores=np.ones((3, 59), F32)), "video bad: user_summary spans 60 frames, user_scores 59"),
    "33 summaries": (dict(user_summary=np.ones((33, 60), F32)), r"video bad has 33 annotators in user_summary \(at most 32\)"),
    "33 score rows": (dict(user_scores=np.ones((33, 60), F32)), r"video bad has 33 annotators in user_scores \(at most 32\)"),
    "33 score rows of a long video": (dict(user_summary=None, user_scores=np.ones((33, 16385), F32)), r"video bad has 33 annotators in user_scores"),
    "no frames": (dict(user_summary=np.ones((3, 0), F32), user_scores=None), r"video bad has 0 frames \(1 .. 16777216\)"),
}


class _ReachedTheGpu(Exception):
    pass


def _tripwires(monkeypatch):
    """A machine with a GPU, as far as human_agreement can tell, on which any upload or chain construction raises _ReachedTheGpu."""
    def reached(*a, **k):
        raise _ReachedTheGpu()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(M, "AgreementChain", reached)
    monkeypatch.setattr(torch, "empty", reached)
    monkeypatch.setattr(torch, "from_numpy", reached)


def test_valid_videos_pass_every_host_check(monkeypatch):
    """The control of the refusals below: videos without a defect get as far as the first upload -- a video past MAX_RANK_FRAMES included."""
    _tripwires(monkeypatch)
    with pytest.raises(_ReachedTheGpu):
        M.human_agreement({"good": _video(), "bad": _video(user_scores=None)})
    with pytest.raises(_ReachedTheGpu):
        M.human_agreement({"long": _video(n_frames=16385), "scores only": _video(user_summary=None)}, metric="kendalltau")


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_human_agreement_refuses_on_the_host(name, monkeypatch):
    _tripwires(monkeypatch)
    over, text = REFUSALS[name]
    with pytest.raises(SumkError, match=text):
        M.human_agreement({"good": _video(), "bad": _video(**over)})


def test_human_agreement_refuses_options(monkeypatch):
    _tripwires(monkeypatch)
    with pytest.raises(KeyError, match="metric"):
        M.human_agreement({"v": _video()}, metric="pearson")
    with pytest.raises(SumkError, match="no videos"):
        M.human_agreement({})
    with pytest.raises(SumkError, match="at most 16384"):
        M.rank_users_device(np.ones((2, 16385), F32))
    with pytest.raises(SumkError, match="at most 32"):
        M.rank_users_device(np.ones((33, 10), F32))
    with pytest.raises(SumkError, match="finite"):
        M.rank_users_device(np.full((2, 10), np.nan, F32))


def test_without_a_gpu_says_so(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(M, "AgreementChain", None)
    with pytest.raises(SumkError, match="no GPU"):
        M.human_agreement({"good": _video()})
    with pytest.raises(SumkError, match="no GPU"):
        M.rank_users_device(np.ones((2, 10), F32))


def test_refusal_names_the_limit():
    assert M.refusal(20, 20, 4494) is None and M.refusal(32, 0, 1 << 24) is None and M.refusal(0, 32, 16384) is None
    assert "user_summary" in M.refusal(33, 2, 100) and "user_scores" in M.refusal(2, 33, 100)
    assert "frames" in M.refusal(2, 0, (1 << 24) + 1) and "frames" in M.refusal(2, 2, 0) and "16384" in M.refusal(2, 2, 16385)


# ------------------------------------------------------------------------------------------------ what the C entries refuse on the host copy
FAKE = 0x1000
BIG = 1 << 40


def _descriptors(n, **over):
    d = (_lib.AgreementVideo * n)()
    for e in d:
        e.user_summary = e.user_scores = FAKE
        e.n_frames, e.n_sum, e.n_sc = 60, 3, 3
        for k, v in over.items():
            setattr(e, k, v)
    return d


def _rank(d, totals=(BIG, BIG), null=()):
    """The three entries with made-up non-null pointers, for calls that are REFUSED: every check is made on the host copy of the descriptors,
    before any HIP call, so the answer needs no GPU and nothing is launched.  Never pass arguments that would be accepted."""
    lib = _lib.load()
    p = [None if i in null else FAKE for i in range(6)]
    rc = lib.sumk_rank_rows(p[0], C.cast(d, C.c_void_p), len(d), p[1], p[2], totals[0], p[3], p[4], p[5], totals[1], None)
    return rc, lib.sumk_last_error().decode(errors="replace")


def _f(d, totals=(BIG, BIG), null=()):
    lib = _lib.load()
    p = [None if i in null else FAKE for i in range(6)]
    rc = lib.sumk_agreement_f(p[0], C.cast(d, C.c_void_p), len(d), p[1], totals[0], p[2], p[3], totals[1], p[4], p[5], None)
    return rc, lib.sumk_last_error().decode(errors="replace")


def _corr(d, metric=0, totals=(BIG, BIG, BIG), null=()):
    lib = _lib.load()
    p = [None if i in null else FAKE for i in range(8)]
    rc = lib.sumk_agreement_corr(p[0], C.cast(d, C.c_void_p), len(d), metric, p[1], p[2], totals[0], p[3], p[4], totals[1], p[5], totals[2], None,
                                 p[6], p[7], None)
    return rc, lib.sumk_last_error().decode(errors="replace")


def test_rank_rows_refuses_on_the_host_copy():
    for over, text in ((dict(reserved=1), "reserved"), (dict(n_sc=33), "33 score rows"), (dict(n_sc=-1), "-1 score rows"), (dict(n_frames=16385), "at most 16384"),
                       (dict(n_frames=0), "0 frames"), (dict(user_scores=None), "null user_scores"), (dict(rank0=-1), "ranks"), (dict(row0=BIG), "rows"),
                       (dict(rank0=BIG - 100), "ranks")):
        rc, err = _rank(_descriptors(2, **over))
        assert rc == -1 and text in err, (over, err)
    for i in range(6):
        rc, err = _rank(_descriptors(1), null=(i,))
        assert rc == -1 and "null pointer" in err, (i, err)
    assert _rank(_descriptors(1), totals=(-1, BIG))[0] == -1
    rc, err = _rank(_descriptors(65536))
    assert rc == -1 and "65536 videos" in err, err
    lib = _lib.load()
    assert lib.sumk_rank_rows(FAKE, FAKE, -1, FAKE, FAKE, 0, FAKE, FAKE, FAKE, 0, None) == -1


def test_agreement_f_refuses_on_the_host_copy():
    for over, text in ((dict(reserved=7), "reserved"), (dict(n_sum=33), "33 summaries"), (dict(n_sum=-2), "-2 summaries"), (dict(n_frames=(1 << 24) + 1), "frames"),
                       (dict(n_frames=-5), "frames"), (dict(user_summary=None), "null user_summary"), (dict(f0=-1), "F ["), (dict(f0=BIG - 8), "F ["),
                       (dict(sum0=BIG - 2), "annotators [")):
        rc, err = _f(_descriptors(2, **over))
        assert rc == -1 and text in err, (over, err)
    for i in range(6):
        rc, err = _f(_descriptors(1), null=(i,))
        assert rc == -1 and "null pointer" in err, (i, err)
    assert _f(_descriptors(1), totals=(BIG, -1))[0] == -1
    rc, err = _f(_descriptors(65536))
    assert rc == -1 and "65536 videos" in err, err


def test_agreement_corr_refuses_on_the_host_copy():
    for over, text in ((dict(reserved=1), "reserved"), (dict(n_sc=33), "33 score rows"), (dict(n_frames=16385), "at most 16384"), (dict(rank0=-1), "ranks"),
                       (dict(row0=-1), "rows"), (dict(c0=-1), "C ["), (dict(c0=BIG - 8), "C [")):
        for metric in (0, 1, 2):
            rc, err = _corr(_descriptors(2, **over), metric)
            assert rc == -1 and text in err, (over, err)
    rc, err = _corr(_descriptors(1), metric=3)
    assert rc == -1 and "metric 3" in err, err
    for i in range(8):
        rc, err = _corr(_descriptors(1), null=(i,))
        assert rc == -1 and "null pointer" in err, (i, err)
    assert _corr(_descriptors(1), totals=(BIG, BIG, -1))[0] == -1
    rc, err = _corr(_descriptors(65536))
    assert rc == -1 and "65536 videos" in err, err
