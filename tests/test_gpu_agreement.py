"""GPU: the inter-annotator agreement chain (csrc/agreement.hip through summarizer_amd/utils/agreement.py) against its specification,
tests/agreement_ref.py.  Everything integer or float32 is compared exactly, and so are the float64 results whose operations the
specification fixes (the Spearman numerator and ssq are exact sums; tau follows from integer counts by three operations).  Against scipy
itself both correlations are held to the gates of tests/test_host_eval.py (Spearman: rtol 1e-12, atol 1e-15) and
tests/test_host_kendall.py (Kendall: rtol 1e-13, atol 1e-14); the worst distance per metric is printed and kept in REPORT (written to
$SUMK_REPORT_DIR/agreement.json when set)."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import agreement_ref as R
from summarizer_amd.utils import agreement as M
from summarizer_amd.utils import eval as E
from summarizer_amd.utils import eval_native

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
GATES = {"spearmanr": dict(rtol=1e-12, atol=1e-15), "kendalltau": dict(rtol=1e-13, atol=1e-14)}
REPORT = {"spearmanr": 0.0, "kendalltau": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("AGREEMENT-REPORT worst |device - scipy|", json.dumps(REPORT))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "agreement.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _up(x):
    return None if x is None else torch.from_numpy(np.array(x, dtype=F32)).to(_dev())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    a, b = a.reshape(-1), b.reshape(-1)
    if a.dtype.kind == "f":                                       # bit for bit, a NaN for a NaN (its sign and payload are not specified)
        nan = np.isnan(a)
        assert_array_equal(nan, np.isnan(b), err_msg=what)
        a, b = a[~nan], b[~nan]
    assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _against_scipy(C, x, metric):
    want = R.scipy_matrix(x, metric)
    both = np.isfinite(want) & np.isfinite(C)
    if both.any():
        worst = float(np.abs(C - want)[both].max())
        REPORT[metric] = max(REPORT[metric], worst)
        print(f"AGREEMENT-REPORT {metric} {x.shape}: worst |device - scipy| = {worst:.3e}")
    np.testing.assert_allclose(C, want, **GATES[metric])


# ------------------------------------------------------------------------------------------------ sumk_rank_rows
def _rank_rows_input(n):
    rng = np.random.default_rng(100 + n)
    distinct = (rng.permutation(n).astype(F32) / F32(16384)).astype(F32)
    graded = R.graded(1, n, n)[0]
    zeros = np.where(rng.random(n) < 0.5, F32(-0.0), F32(0.0)).astype(F32)
    zeros[rng.random(n) < 0.3] = F32(-1.5)
    return np.stack([distinct, graded, np.full(n, 0.25, F32), zeros])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1025, 4494, 16384])
def test_rank_rows_equal_the_host_metadata(n):
    """All-distinct, five-grade, all-equal and -0.0 / 0.0 rows: the ranks of eval.rank_users, the dense ranks and tie counts of
    eval_native._kendall_meta, numpy's mean and ssq -- exactly."""
    x = _rank_rows_input(n)
    ranks, meta = M.rank_users_device(x)
    ru = E.rank_users(x)
    _same(ranks, ru, "ranks")
    dense, ytie = eval_native._kendall_meta({"user_ranks": ru})
    _same(meta["dense"], dense, "dense"); _same(meta["ties"], ytie, "ties")
    mu = ru.sum(axis=1) / ru.shape[1]
    _same(meta["mean"], mu, "mean"); _same(meta["mean"], ru.mean(axis=1), "np.mean")
    _same(meta["ssq"], ((ru - mu[:, None]) ** 2).sum(axis=1), "ssq")
    spec = R.rank_rows(x)
    for k in ("dense", "ties", "mean", "ssq"):
        _same(meta[k], spec[k], k)
    # a device tensor in: device tensors out, the same values
    r2, m2 = M.rank_users_device(_up(x))
    assert r2.is_cuda and m2["dense"].is_cuda
    _same(r2.cpu().numpy(), ru); _same(m2["ties"].cpu().numpy(), ytie)


# ------------------------------------------------------------------------------------------------ sumk_agreement_f
F_USERS = (1, 2, 3, 7, 8, 9, 20, 32)


@functools.lru_cache(maxsize=None)
def _f_case(n):
    vids = []
    for U in F_USERS:
        us = R.selections(U, n, 1000 * U + n, density=0.3 if n > 1 else 0.7)
        if U >= 3:
            us[1] = 0                                             # an empty summary
            us[2] = us[0]                                         # two identical summaries
        us.setflags(write=False)
        vids.append(us)
    return vids, [R.f_agreement(us) for us in vids]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4494, 70000])
def test_f_scores_equal_the_specification(n):
    vids, want = _f_case(n)
    chain = M.AgreementChain([_up(us) for us in vids], [None] * len(vids), "spearmanr")
    chain.nan_fill()
    chain.enqueue()
    got = chain.views(chain.to_host())
    for U, g, w in zip(F_USERS, got, want):
        for k in ("F", "f_avg_user", "f_max_user"):
            _same(g[k], w[k], f"U={U} {k}")
        _same(F64(g["f_avg"]), w["f_avg"], f"U={U} f_avg"); _same(F64(g["f_max"]), w["f_max"], f"U={U} f_max")
        assert np.isnan(g["corr"])
        _same(g["F"], g["F"].T.copy(), "F is symmetric")
        if U >= 3:
            assert g["F"][0, 2] == (1 if vids[F_USERS.index(U)][0].any() else 0) and not g["F"][1].any()
    assert np.isnan(got[0]["f_avg"]) and np.isnan(got[0]["f_max_user"]).all()


# ------------------------------------------------------------------------------------------------ sumk_agreement_corr
CORR_CASES = [(2, 2), (3, 3), (32, 3), (2, 1024), (20, 1024), (32, 1025), (20, 4494), (3, 16384), (2, 16384)]


@functools.lru_cache(maxsize=None)
def _corr_case(U, n):
    """Half the rows graded (five values: heavy ties), half continuous; from four rows up one constant row (index 1) and two equal rows
    (the last = the first)."""
    x = np.concatenate([R.graded((U + 1) // 2, n, 7 * U + n), R.continuous(U // 2, n, 11 * U + n)])
    if U >= 4:
        x[1] = F32(0.5)
        x[U - 1] = x[0]
    x.setflags(write=False)
    return x, {m: R.corr_agreement(x, m) for m in M.METRICS}


@pytest.mark.parametrize("U,n", CORR_CASES)
@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_correlations_equal_the_specification(U, n, metric):
    x, want = _corr_case(U, n)
    w = want[metric]
    chain = M.AgreementChain([None], [_up(x)], metric)
    chain.nan_fill()
    chain.enqueue()
    g = chain.views(chain.to_host())[0]
    if metric == "kendalltau":
        _same(g["counts"], w["counts"], "counts")
        tot = n * (n - 1) // 2
        tau = np.array([[R.kendall_tau_b(*([int(g["counts"][a, b, 0]), tot] + [int(t) for t in g["counts"][a, b, 1:3]])) for b in range(U)] for a in range(U)])
        _same(g["C"], tau.reshape(U, U), "tau from the counts")
    _same(g["C"], w["C"], "C"); _same(g["corr_user"], w["corr_user"], "corr_user"); _same(F64(g["corr"]), w["corr"], "corr")
    assert np.isnan(g["f_avg"]) and np.isnan(g["f_max"])
    _against_scipy(g["C"], x, metric)
    if U >= 4:
        assert np.isnan(g["C"][1]).all() and np.isnan(g["C"][:, 1]).all() and np.isnan(g["corr"])
        assert abs(g["C"][0, U - 1] - 1.0) <= 2.3e-16 and abs(g["C"][U - 1, 0] - 1.0) <= 2.3e-16
    if metric == "spearmanr":
        _same(g["C"], g["C"].T.copy(), "rho is symmetric")


def _levels(n, k, seed):
    """A row of exactly k distinct values (every value occurs)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.arange(k), rng.integers(0, k, size=n - k)]).astype(F32)
    rng.shuffle(x)
    return x


@pytest.mark.parametrize("case", ["graded 20 x 4494", "mixed 32 x 1025", "32 and 33 levels", "one frame each side of a slice"])
def test_kendall_table_and_sort_paths_agree(case):
    """Pairs of rows with few distinct values take their counts from a contingency table (their product at most 1024), the others from
    the sort; SUMK_AGREEMENT_KENDALL_SORT sends every pair through the sort.  The same rows either way: the same integers, the same tau --
    and the specification's.  32 x 32 levels is the last table, 32 x 33 the first sort."""
    if case == "graded 20 x 4494":
        x = _corr_case(20, 4494)[0]
    elif case == "mixed 32 x 1025":
        x = _corr_case(32, 1025)[0]
    elif case == "32 and 33 levels":
        x = np.stack([_levels(3000, 32, 1), _levels(3000, 32, 2), _levels(3000, 33, 3), _levels(3000, 1, 4), _levels(3000, 2, 5)])
    else:
        x = np.stack([_levels(n_, k, 6 + k) for n_, k in ((1025, 5), (1025, 7), (1025, 3))])
    got = []
    for sort_only in (False, True):
        chain = M.AgreementChain([None], [_up(x)], "kendalltau", _sort_only=sort_only)
        chain.enqueue()
        got.append(chain.views(chain.to_host())[0])
    for k in ("counts", "C", "corr_user"):
        _same(got[0][k], got[1][k], k)
    _same(got[0]["corr"], got[1]["corr"])
    want = R.corr_agreement(x, "kendalltau")
    _same(got[0]["counts"], want["counts"]); _same(got[0]["C"], want["C"])


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_two_equal_rows_and_a_constant_row_among_three(metric):
    x = R.continuous(3, 1024, 77)
    x[2] = x[0]
    g = M.human_agreement({"v": {"user_scores": x}}, metric)["videos"]["v"]
    assert abs(g["C"][0, 2] - 1.0) <= 2.3e-16 and np.isfinite(g["corr"])
    _same(g["C"], R.corr_agreement(x, metric)["C"])
    x[1] = F32(2)
    g = M.human_agreement({"v": {"user_scores": x}}, metric)["videos"]["v"]
    assert np.isnan(g["C"][1]).all() and np.isnan(g["C"][:, 1]).all() and np.isnan(g["corr_user"]).all() and np.isnan(g["corr"])
    _same(g["C"], R.corr_agreement(x, metric)["C"])


# ------------------------------------------------------------------------------------------------ a ragged batch through human_agreement
@functools.lru_cache(maxsize=None)
def _batch():
    vids = {
        "both": {"user_summary": R.selections(5, 300, 1), "user_scores": R.graded(5, 300, 2)},
        "scores only": {"user_scores": R.continuous(3, 1025, 3)},
        "summary only": {"user_summary": R.selections(7, 4494, 4)},
        "long": {"user_summary": R.selections(4, 20000, 5), "user_scores": R.graded(3, 20000, 6)},
        "many scorers": {"user_summary": R.selections(2, 64, 7), "user_scores": R.graded(20, 64, 8)},
        "many summaries": {"user_summary": R.selections(32, 33, 9), "user_scores": R.continuous(2, 33, 10)},
    }
    return vids, {m: {k: R.agreement(v.get("user_summary"), v.get("user_scores"), m) for k, v in vids.items()} for m in M.METRICS}


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_ragged_batch(metric):
    vids, want = _batch()
    got = M.human_agreement(vids, metric)
    f_avg, f_max, corr = [], [], []
    for k, v in vids.items():
        g, w = got["videos"][k], want[metric][k]
        assert g["path"] == ("host" if k == "long" else "device")
        if "user_summary" in v:
            for name in ("F", "f_avg_user", "f_max_user"):
                _same(g[name], w[name], f"{k} {name}")
            _same(F64(g["f_avg"]), w["f_avg"]); _same(F64(g["f_max"]), w["f_max"])
            f_avg.append(w["f_avg"]); f_max.append(w["f_max"])
        else:
            assert np.isnan(g["f_avg"]) and np.isnan(g["f_max"]) and g["F"].shape == (0, 0)
        if "user_scores" not in v:
            assert np.isnan(g["corr"]) and g["C"].shape == (0, 0)
        elif k == "long":                                         # the host functions of utils/eval.py: within the scipy gates
            np.testing.assert_allclose(g["C"], w["C"], **GATES[metric])
            np.testing.assert_allclose(g["corr_user"], w["corr_user"], **GATES[metric])
            np.testing.assert_allclose(g["corr"], w["corr"], **GATES[metric])
            _against_scipy(g["C"], v["user_scores"], metric)
            corr.append(g["corr"])
        else:
            _same(g["C"], w["C"], f"{k} C"); _same(g["corr_user"], w["corr_user"]); _same(F64(g["corr"]), w["corr"])
            corr.append(w["corr"])
    assert got["f_avg"] == float(np.mean(f_avg)) and got["f_max"] == float(np.mean(f_max)) and got["corr"] == float(np.mean(corr))
    assert got["result"] == (got["corr"], (got["f_avg"], got["f_max"]))
    # device=True: device tensors, the same values; device tensors in: the same values again
    on_dev = M.human_agreement({k: {f: _up(a) for f, a in v.items()} for k, v in vids.items()}, metric, device=True)
    assert on_dev["result"] is None and on_dev["corr"].is_cuda and on_dev["f_avg"].shape == (5,) and on_dev["corr"].shape == (5,)
    for k in vids:
        g, d = got["videos"][k], on_dev["videos"][k]
        assert d["path"] == g["path"]
        for name in ("f_avg", "f_max", "corr", "f_avg_user", "f_max_user", "corr_user", "F", "C"):
            assert torch.is_tensor(d[name]) and d[name].is_cuda, (k, name)
            _same(d[name].cpu().numpy(), np.asarray(g[name]), f"{k} {name} device=True")


# ------------------------------------------------------------------------------------------------ robustness
def _small_batch():
    vids, _ = _batch()
    keys = ["both", "scores only", "summary only", "many scorers", "many summaries"]
    return [_up(vids[k].get("user_summary")) for k in keys], [_up(vids[k].get("user_scores")) for k in keys]


def _declared(chain, carve, names):
    """Byte mask of what the chain declares as its outputs inside one allocation."""
    lay = {"ties": ("row", 1), "mean": ("row", 1), "ssq": ("row", 1), "corr_user": ("row", 1), "C": ("C", 1), "counts": ("C", 4), "F": ("F", 1),
           "f_avg_user": ("sum", 1), "f_max_user": ("sum", 1), "ranks": ("rank", 1), "dense": ("rank", 1)}
    total = max(a + nb for a, nb, _ in carve.values())
    mask = np.zeros(total, bool)
    for name in names:
        a, nb, dt = carve[name]
        size = torch.empty(0, dtype=dt).element_size()
        if name in ("f_avg", "f_max", "corr"):
            mask[a:a + nb] = True
            continue
        which, k = lay[name]
        for at, count in chain.layout[which]:
            mask[a + k * at * size:a + k * (at + count) * size] = True
    return mask


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_poisoned_buffers_and_guard_regions(metric):
    """Every output and scratch buffer pre-filled with 0xFF bytes: the same results as on zeroed buffers, and no byte outside the declared
    outputs touched -- the gaps behind every video's range and the padding between the buffers are the guard regions."""
    summ, sc = _small_batch()
    runs = []
    for fill in (0, 255):
        chain = M.AgreementChain(summ, sc, metric, _gap=5)
        chain.arena.fill_(fill); chain.scratch.fill_(fill)
        chain.enqueue()
        torch.cuda.synchronize()
        runs.append((chain, chain.arena.cpu().numpy().copy(), chain.scratch.cpu().numpy().copy()))
    (chain, a0, s0), (_, a1, s1) = runs
    ma, ms = _declared(chain, chain._carve, list(chain._carve)), _declared(chain, chain._scarve, list(chain._scarve))
    assert ma.any() and ms.any() and not ma.all() and not ms.all()
    assert_array_equal(a0[:ma.size][ma], a1[:ma.size][ma]); assert_array_equal(s0[:ms.size][ms], s1[:ms.size][ms])
    assert (a1[:ma.size][~ma] == 255).all() and (a1[ma.size:] == 255).all() and (a0[:ma.size][~ma] == 0).all()
    assert (s1[:ms.size][~ms] == 255).all() and (s1[ms.size:] == 255).all() and (s0[:ms.size][~ms] == 0).all()
    # and the values are the specification's
    vids, want = _batch()
    views = chain.views({name: a0[a:a + nb].view(M._NP[dt]) for name, (a, nb, dt) in chain._carve.items()})
    for k, g in zip(["both", "scores only", "summary only", "many scorers", "many summaries"], views):
        w = want[metric][k]
        if "F" in w:
            _same(g["F"], w["F"]); _same(F64(g["f_avg"]), w["f_avg"])
        if "C" in w:
            _same(g["C"], w["C"]); _same(F64(g["corr"]), w["corr"])


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_chain_replays_from_a_graph(metric):
    """One capture of the three enqueued calls on fixed buffers, two replays: the eager results, byte for byte."""
    summ, sc = _small_batch()
    chain = M.AgreementChain(summ, sc, metric)
    chain.enqueue()
    torch.cuda.synchronize()
    eager = (chain.arena.cpu().numpy().copy(), chain.scratch.cpu().numpy().copy())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain.enqueue()
    for _ in range(2):
        chain.arena.fill_(255); chain.scratch.fill_(255)
        g.replay()
        torch.cuda.synchronize()
        ma, ms = _declared(chain, chain._carve, list(chain._carve)), _declared(chain, chain._scarve, list(chain._scarve))
        a, s = chain.arena.cpu().numpy(), chain.scratch.cpu().numpy()
        assert_array_equal(a[:ma.size][ma], eager[0][:ma.size][ma]); assert_array_equal(s[:ms.size][ms], eager[1][:ms.size][ms])


# ------------------------------------------------------------------------------------------------ Trainer
def test_trainer_human_agreement_is_human_agreement_on_the_fold():
    from types import SimpleNamespace
    from summarizer_amd.models import Trainer
    from summarizer_amd.utils.datasets import synthetic_dataset
    ds = synthetic_dataset(4, seed=3, D=8, t_range=(20, 40), n_users=6)
    keys = list(ds.keys())
    hps = SimpleNamespace(logger=None, dataset_of_file={"s": ds}, dataset_name_of_file={"s": "synthetic"}, correlation_metric="kendalltau",
                          splits_of_file={"s": [{"train_keys": keys[:1], "test_keys": keys[1:]}]})
    t = Trainer(hps, "s")
    for metric, name in ((None, "kendalltau"), ("spearmanr", "spearmanr")):
        got = t.human_agreement(0, metric)
        want = M.human_agreement({k: ds[k] for k in keys[1:]}, name)
        assert got["result"] == want["result"] and list(got["videos"]) == keys[1:] and np.isfinite(got["result"][0])
        for k in keys[1:]:
            _same(got["videos"][k]["C"], want["videos"][k]["C"]); _same(got["videos"][k]["F"], want["videos"][k]["F"])
            spec = R.agreement(ds[k]["user_summary"][...], ds[k]["user_scores"][...], name)
            _same(got["videos"][k]["C"], spec["C"]); _same(got["videos"][k]["F"], spec["F"])
    assert not hasattr(t, "fold")


def test_command_line_prints_the_human_row(tmp_path, capsys):
    vids, want = _batch()
    keys = ["both", "many scorers"]
    path = str(tmp_path / "data.npz")
    np.savez(path, **{f"{k}/{f}": a for k in keys for f, a in vids[k].items()})
    assert M.main([path, "--metric", "kendalltau"]) == 0
    w = [want["kendalltau"][k] for k in keys]
    row = {"videos": keys, "f_avg": float(np.mean([x["f_avg"] for x in w])), "f_max": float(np.mean([x["f_max"] for x in w])),
           "corr": float(np.mean([x["corr"] for x in w]))}
    assert capsys.readouterr().out.strip() == M.table_row(row, "kendalltau")
