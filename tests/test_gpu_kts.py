"""GPU: kernel temporal segmentation on the device (csrc/kts.hip: sumk_kts, sumk_kts_gram, sumk_kts_gram_nonlin), utils.kts, Summarizer and
the Trainer opt-in, against the float64 numpy reference tests/kts_ref.py (pinned against brute force in tests/test_kts_host.py).

Gates
  * from a float64 Gram matrix (sumk_kts_gram) both sides start from the same float64 input and only the summation order differs:
    n_cps and cps EQUAL, finite scores within 1e-9 * max(1, |score|), the infinite sets equal.
  * from features (sumk_kts) the Gram matrix is exact fp32 on the device.  The float64 reference on the float64 Gram is the reference, the
    SAME reference on numpy's float32 Gram is the yardstick (largest |difference| of the scores over k); the device scores must stay within
    4 x the yardstick, with a floor of 2 fp32 ulps (2^-24 relative) of the largest score.  Change points and m_best must be EQUAL in every
    case; the test first asserts on the reference alone that the best and the second-best cost differ by more than 100 x gate / n, so an
    fp32-sized perturbation of the scores cannot change the choice.
The worst error / gate of every case is printed and kept in REPORT (written to $SUMK_REPORT_DIR/kts_f64.json when set).

Figures: NOT MEASURED on an MI355X at the time of writing, so no worst ratio is quoted.  On the CPU (reference against reference, no kernel
involved) the planted cases have yardsticks 6.6e-7 .. 2.8e-6 and gates 2.7e-6 .. 2.7e-5 (the 2-ulp floor decides from n = 130 on) against
cost margins of 6.3e-3 .. 3.9e-2; the unstructured cases (seeds 11-13, m_best = 12) yardsticks 7.6e-6 .. 1.1e-4, gates 1e-3 (the floor: scores
~8e3) against margins of 0.6; the float32-Gram reference returns the float64 one's change points in every case.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import kts_ref

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -24
REPORT = []
PLANTED_SEGS = {33: 3, 65: 5, 130: 7, 200: 8, 257: 9}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for r in REPORT:
        print("KTS-F64-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "kts_f64.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


# ------------------------------------------------------------------------------------------------ inputs and references (computed once)
@functools.lru_cache(maxsize=None)
def _gram(n, seed=0):
    """float64 Gram matrix of n L2-normalised random rows (entries <= 1: the reference's own 2-D prefix sums stay ~1e-13 accurate)."""
    rng = np.random.default_rng(1000 * seed + n)
    X = rng.standard_normal((n, 8))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    K = X @ X.T
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def _ref_auto(n, max_ncp, vmax=1.0, lmin=1, lmax=100000):
    return kts_ref.cpd_auto(_gram(n), max_ncp, vmax, lmin, lmax, full=True)


def _raw_call(dev, name, src, lens, D, max_ncp, lmin=1, lmax=100000, vmax=1.0, fill=False, ws_bytes=None):
    """The C entry itself on buffers of this test (fill: workspace and outputs handed over as 0xFF bytes).  Returns (rc, n_cps, cps, scores)."""
    from summarizer_amd import _lib
    lib = _lib.load()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    off_dev = torch.from_numpy(off).to(dev)
    need = lib.sumk_kts_workspace_bytes(4 if name != "sumk_kts" else D, len(lens), _lib.host_i32(off), max_ncp)
    nb = need if ws_bytes is None else ws_bytes
    ws =torch.full((max(nb, 256),), 255, dtype=torch.uint8, device=dev) if fill else torch.zeros(max(nb, 256), dtype=torch.uint8, device=dev)
    n_cps = torch.full((len(lens),), -7, dtype=torch.int32, device=dev)
    cps = torch.full((len(lens), max(max_ncp, 1)), -7, dtype=torch.int32, device=dev)
    scores = torch.full((len(lens), max(max_ncp, 0) + 1), float("nan"), dtype=torch.float64, device=dev)
    if fill:
        for t in (n_cps, cps, scores):
            t.view(torch.uint8).fill_(255)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tail = (p(n_cps), p(cps), p(scores), p(ws), nb, st)
    if name == "sumk_kts":
        rc = lib.sumk_kts(p(src), D, len(lens), _lib.host_i32(off), p(off_dev), max_ncp, lmin, lmax, float(vmax), *tail)
    elif name == "sumk_kts_gram":
        rc = lib.sumk_kts_gram(p(src), len(lens), _lib.host_i32(off), p(off_dev), max_ncp, lmin, lmax, float(vmax), *tail)
    else:
        rc = lib.sumk_kts_gram_nonlin(p(src), len(lens), _lib.host_i32(off), p(off_dev), max_ncp, lmin, lmax, *tail)
    torch.cuda.synchronize()
    return rc, n_cps.cpu().numpy(), cps.cpu().numpy()[:, :max(max_ncp, 0)], scores.cpu().numpy(), need


def _flat(dev, Ks):
    return torch.from_numpy(np.concatenate([np.asarray(K, dtype=np.float64).reshape(-1) for K in Ks])).to(dev)


def _check_exact(tag, n, max_ncp, got, ref, tol_rel=1e-9, tol_abs=None):
    """got = (n_cps, cps row (max_ncp,), scores row (max_ncp + 1,)) of one video; ref = (mb, cps, s, cost) of kts_ref.cpd_auto(full=True)."""
    n_cps, cps, scores = got
    mb, rcps, s, _ = ref
    assert n_cps == mb, (tag, n, n_cps, mb)
    assert np.array_equal(cps[:mb], rcps), (tag, n, cps[:mb].tolist(), rcps.tolist())
    assert (cps[mb:] == -1).all(), (tag, n)
    want = np.full(max_ncp + 1, np.inf)
    want[:mb + 1] = s[:mb + 1]
    assert np.array_equal(np.isinf(scores), np.isinf(want)) and not np.isnan(scores).any(), (tag, n, scores, want)
    fin = np.isfinite(want)
    err = np.abs(scores[fin] - want[fin])
    tol = tol_rel * np.maximum(1.0, np.abs(want[fin])) if tol_abs is None else tol_abs
    assert (err <= tol).all(), (tag, n, float(err.max()))
    return float(err.max()) if err.size else 0.0


# ------------------------------------------------------------------------------------------------ 1. the DP from a float64 Gram
@pytest.mark.parametrize("n,max_ncp", [(1, 0), (2, 1), (3, 2), (33, 32), (64, 63), (65, 64), (130, 129), (257, 256), (1025, 40)])
def test_dp_from_float64_gram(dev, n, max_ncp):
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get([n], dev)
    n_cps, cps, scores = kernels.kts_gram(_flat(dev, [_gram(n)]), sb, max_ncp)
    err = _check_exact("gram", n, max_ncp, (int(n_cps[0]), cps[0].cpu().numpy(), scores[0].cpu().numpy()), _ref_auto(n, max_ncp))
    print("KTS gram n", n, "max_ncp", max_ncp, "m_best", int(n_cps[0]), "max |score error|", err)


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("opt", ["lmin4_lmax40", "infeasible_tail", "vmax0.25", "vmax4"])
def test_dp_options(dev, n, opt):
    from summarizer_amd import kernels
    kw = {"lmin4_lmax40": dict(lmin=4, lmax=40), "infeasible_tail": dict(lmin=10), "vmax0.25": dict(vmax=0.25), "vmax4": dict(vmax=4.0)}[opt]
    max_ncp = n - 1
    sb = kernels.SeqBatch.get([n], dev)
    K = _flat(dev, [_gram(n)])
    ref = _ref_auto(n, max_ncp, kw.get("vmax", 1.0), kw.get("lmin", 1), kw.get("lmax", 100000))
    n_cps, cps, scores = kernels.kts_gram(K, sb, max_ncp, **kw)
    _check_exact(opt, n, max_ncp, (int(n_cps[0]), cps[0].cpu().numpy(), scores[0].cpu().numpy()), ref)
    if opt == "lmin4_lmax40":
        seg = np.diff(np.concatenate([[0], ref[1], [n]]))
        assert seg.max() <= 40 and ref[0] >= 1
    if opt == "infeasible_tail":
        # (k + 1) * lmin > n from k = n // 10 on: those rows are +inf in the reference and can never be chosen; the fixed-m entry shows the
        # whole row, the infeasible part included, and its backtrack from an infeasible row (all zeros in the original's table)
        first_bad = n // 10
        assert np.isinf(ref[2][first_bad:]).all() and np.isfinite(ref[2][:first_bad]).all() and ref[0] < first_bad
        ncp = first_bad + 2
        rcps, rs = kts_ref.cpd_nonlin(_gram(n), ncp, lmin=10)
        m_fix, cps_fix, s_fix = kernels.kts_gram_nonlin(K, sb, ncp, lmin=10)
        s_fix = s_fix[0].cpu().numpy()
        assert int(m_fix[0]) == ncp and np.array_equal(cps_fix[0].cpu().numpy(), rcps)
        assert np.array_equal(np.isinf(s_fix), np.isinf(rs)) and np.isinf(s_fix[first_bad:]).all()
        fin = np.isfinite(rs)
        assert (np.abs(s_fix[fin] - rs[fin]) <= 1e-9 * np.maximum(1.0, np.abs(rs[fin]))).all()
        # and a feasible fixed m: cpd_nonlin proper
        rcps, rs = kts_ref.cpd_nonlin(_gram(n), first_bad - 1, lmin=10)
        m_fix, cps_fix, s_fix = kernels.kts_gram_nonlin(K, sb, first_bad - 1, lmin=10)
        assert int(m_fix[0]) == first_bad - 1 and np.array_equal(cps_fix[0].cpu().numpy(), rcps)
        assert (np.abs(s_fix[0].cpu().numpy() - rs) <= 1e-9 * np.maximum(1.0, np.abs(rs))).all()


RAGGED = [1, 2, 65, 130, 33]


def _ragged(dev, fill):
    max_ncp = max(RAGGED) - 1
    rc, n_cps, cps, scores, _ = _raw_call(dev, "sumk_kts_gram", _flat(dev, [_gram(n) for n in RAGGED]), RAGGED, 4, max_ncp, fill=fill)
    assert rc == 0
    return max_ncp, n_cps, cps, scores


def test_ragged_batch_on_poisoned_buffers(dev):
    max_ncp, n_cps, cps, scores = _ragged(dev, fill=True)
    for v, n in enumerate(RAGGED):
        _check_exact("ragged", n, max_ncp, (int(n_cps[v]), cps[v], scores[v]), _ref_auto(n, max_ncp))
    assert n_cps[0] == 0 and n_cps[1] <= 1


def test_python_cpd_functions(dev):
    from summarizer_amd.utils import kts
    K = _gram(65)
    mb, rcps, s, _ = _ref_auto(65, 64)
    for src in (K, torch.from_numpy(np.array(K)).to(dev)):
        cps, scores = kts.cpd_auto(src, 64)
        assert cps.shape == (mb,) and scores.shape == (mb + 1,) and np.array_equal(cps, rcps)
        np.testing.assert_allclose(scores, s[:mb + 1], rtol=1e-9, atol=1e-9)
    rcps, rs = kts_ref.cpd_nonlin(K, 5)
    cps, scores = kts.cpd_nonlin(K, 5)
    assert cps.shape == (5,) and scores.shape == (6,) and np.array_equal(cps, rcps)
    np.testing.assert_allclose(scores, rs, rtol=1e-9, atol=1e-9)
    with pytest.raises(ValueError):
        kts.cpd_nonlin(K, 65)


# ------------------------------------------------------------------------------------------------ 2. from features
@functools.lru_cache(maxsize=None)
def _feature_case(kind, n, D, seed):
    """(X float32, max_ncp, ref on the float64 Gram, yardstick, gate) -- reference against reference, no kernel involved."""
    if kind == "planted":
        X, _ = kts_ref.planted_features(n, D, PLANTED_SEGS[n], 0.3 if D == 1024 else 0.05, seed)
        max_ncp = n - 1
    else:
        X = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
        max_ncp = 12
    K64 = X.astype(np.float64) @ X.astype(np.float64).T
    K32 = (X @ X.T).astype(np.float64)
    ref = kts_ref.cpd_auto(K64, max_ncp, full=True)
    s64, s32 = ref[2], kts_ref.cpd_auto(K32, max_ncp, full=True)[2]
    fin = np.isfinite(s64)
    assert np.array_equal(fin, np.isfinite(s32))
    yard = float(np.abs(s32 - s64)[fin].max())
    gate = max(4 * yard, 2 * ULP * float(np.abs(s64[fin]).max()))
    X.setflags(write=False)
    return X, max_ncp, ref, K64, yard, gate


def _run_features(dev, X, max_ncp):
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get([X.shape[0]], dev)
    n_cps, cps, scores = kernels.kts(torch.from_numpy(np.array(X)).to(dev), sb, max_ncp)
    return int(n_cps[0]), cps[0].cpu().numpy(), scores[0].cpu().numpy()


@pytest.mark.parametrize("D", [64, 1024])
@pytest.mark.parametrize("n", [33, 65, 130, 200, 257])
def test_from_features_planted(dev, n, D):
    X, max_ncp, ref, _, yard, gate = _feature_case("planted", n, D, 100 + n + D)
    margin = kts_ref.cost_margin(ref[3])
    assert margin > 100 * gate / n, (n, D, margin, gate)                 # on the reference alone: the choice of m is well separated
    got = _run_features(dev, X, max_ncp)
    print("KTS features n", n, "D", D, "m_best", got[0], "ref", ref[0], "yardstick", yard, "gate", gate, "margin", margin)
    err = _check_exact("features", n, max_ncp, got, ref, tol_abs=np.inf)
    REPORT.append({"case": f"planted_n{n}_D{D}", "yardstick": yard, "gate": gate, "error": err, "ratio": err / gate, "cost_margin": margin})
    print("KTS features n", n, "D", D, "max |score error|", err, "error / gate", err / gate)
    _check_exact("features", n, max_ncp, got, ref, tol_abs=gate)


# ------------------------------------------------------------------------------------------------ 3. unstructured input
IID_SEEDS = (11, 12, 13)


@pytest.mark.parametrize("seed", IID_SEEDS)
def test_from_features_unstructured(dev, seed):
    n, D = 130, 64
    X, max_ncp, ref, K64, yard, gate = _feature_case("iid", n, D, seed)
    margin = kts_ref.cost_margin(ref[3])
    assert margin > 100 * gate / n, (seed, margin, gate)
    m, cps, scores = _run_features(dev, X, max_ncp)
    print("KTS iid seed", seed, "m_best", m, "ref", ref[0], "yardstick", yard, "gate", gate, "margin", margin)
    assert m == ref[0]
    # the device's change points at the device's m: their float64 objective against the reference's optimum for that m
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get([n], dev)
    mfix = 7
    _, cps_fix, _ = kernels.kts(torch.from_numpy(np.array(X)).to(dev), sb, mfix, vmax=0.0)      # vmax = 0: the penalty vanishes, m_best = the last row that still lowers the scatter
    cps_fix = cps_fix[0].cpu().numpy()
    for tag, c in (("auto", cps[:m]), ("m7", cps_fix[cps_fix >= 0])):
        k = len(c)
        assert (np.diff(np.concatenate([[0], c, [n]])) >= 1).all()
        obj, opt = kts_ref.objective(K64, c), kts_ref.cpd_nonlin(K64, k)[1][k]
        err = obj - opt
        REPORT.append({"case": f"iid_seed{seed}_{tag}", "m": k, "yardstick": yard, "gate": gate, "error": err, "ratio": abs(err) / gate, "cost_margin": margin})
        print("KTS iid seed", seed, tag, "m", k, "objective - optimum", err, "gate", gate)
        assert -1e-9 * max(1.0, abs(opt)) <= err <= gate, (seed, tag, err, gate)
    fin = np.isfinite(scores)
    assert (np.abs(scores[fin] - ref[2][:len(scores)][fin]) <= gate).all()


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_bit_determinism(dev):
    a, b = _ragged(dev, fill=False), _ragged(dev, fill=True)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3].view(np.int64), b[3].view(np.int64))


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_bad_arguments_are_refused(dev):
    from summarizer_amd import _lib
    lib = _lib.load()
    X, max_ncp, ref, _, _, gate = _feature_case("planted", 33, 64, 100 + 33 + 64)
    x = torch.from_numpy(np.array(X)).to(dev)

    def good():
        rc, n_cps, cps, scores, _ = _raw_call(dev, "sumk_kts", x, [33], 64, max_ncp)
        assert rc == 0
        _check_exact("after refusal", 33, max_ncp, (int(n_cps[0]), cps[0], scores[0]), ref, tol_abs=gate)

    good()
    need = lib.sumk_kts_workspace_bytes(64, 1, _lib.host_i32(np.array([0, 33], dtype=np.int32)), max_ncp)
    x6 = torch.zeros(33, 6, device=dev)
    bad = [("n=16385", dict(lens=[16385], D=64, max_ncp=3)), ("lmin=0", dict(lens=[33], D=64, max_ncp=max_ncp, lmin=0)),
           ("lmax<lmin", dict(lens=[33], D=64, max_ncp=max_ncp, lmin=5, lmax=4)), ("D=6", dict(lens=[33], D=6, max_ncp=max_ncp, src=x6)),
           ("short workspace", dict(lens=[33], D=64, max_ncp=max_ncp, ws_bytes=need - 1)),
           ("max_ncp=n", dict(lens=[33], D=64, max_ncp=33)), ("max_ncp<0", dict(lens=[33], D=64, max_ncp=-1))]
    for tag, kw in bad:
        src = kw.pop("src", x)
        rc, n_cps, _, _, _ = _raw_call(dev, "sumk_kts", src, kw.pop("lens"), kw.pop("D"), kw.pop("max_ncp"), **kw)
        msg = lib.sumk_last_error().decode()
        assert rc == -1 and "kts" in msg and len(msg) > 8, (tag, rc, msg)
        assert (n_cps == -7).all(), tag                                  # nothing was launched
        good()
    Kd = _flat(dev, [_gram(33)])
    for name in ("sumk_kts_gram", "sumk_kts_gram_nonlin"):
        rc = _raw_call(dev, name, Kd, [33], 4, 5, ws_bytes=1024)[0]
        assert rc == -1 and "workspace" in lib.sumk_last_error().decode(), name
        rc = _raw_call(dev, name, Kd, [33], 4, 5, lmin=0)[0]
        assert rc == -1 and "lmin" in lib.sumk_last_error().decode(), name
    good()


# ------------------------------------------------------------------------------------------------ 6. Summarizer
def _irregular_picks(n, seed):
    rng = np.random.default_rng(seed)
    picks = np.cumsum(rng.integers(5, 25, size=n)).astype(np.int32)
    picks -= picks[0]
    return picks, int(picks[-1]) + int(rng.integers(3, 20))


def test_summarizer(dev):
    import summarizer_amd
    from summarizer_amd.models.vasnet import VASNet
    from summarizer_amd.utils import eval as ev
    from summarizer_amd.utils.kts import cps_to_segments
    torch.manual_seed(5)
    model = VASNet(input_size=64).eval().to(dev)
    cases = [_feature_case("planted", n, 64, 100 + n + 64) for n in (65, 130)]
    meta = [_irregular_picks(n, 40 + n) for n in (65, 130)]
    proportion = 0.15
    s = summarizer_amd.Summarizer(model, proportion=proportion, method="knapsack")
    out = s.summarize_batch([torch.from_numpy(np.array(c[0])).to(dev) for c in cases], [m[0] for m in meta], [m[1] for m in meta])
    assert len(out) == 2
    with torch.no_grad():
        packed = torch.cat([torch.from_numpy(np.array(c[0])) for c in cases]).to(dev)
        want_scores = model.score_packed(packed, [65, 130]).reshape(-1).cpu().numpy()
    for (X, max_ncp, ref, _, _, _), (picks, n_frames), o, sc in zip(cases, meta, out, np.split(want_scores, [65])):
        cp, nfps = cps_to_segments(ref[1], picks, n_frames)
        assert o["change_points"].dtype == np.int32 and np.array_equal(o["change_points"], cp) and np.array_equal(o["n_frame_per_seg"], nfps)
        assert np.array_equal(o["scores"], sc) and o["scores"].dtype == np.float32
        summary = ev.generate_summary(o["scores"], cp, n_frames, nfps.tolist(), picks, proportion, "knapsack")
        assert np.array_equal(o["machine_summary"], summary)
        assert len(o["machine_summary"]) == n_frames and o["machine_summary"].sum() <= proportion * n_frames
        assert set(np.unique(o["machine_summary"]).tolist()) <= {0.0, 1.0}
    one = s.summarize(np.array(cases[0][0]), meta[0][0], meta[0][1])                 # one video, host features
    assert np.array_equal(one["change_points"], out[0]["change_points"]) and len(one["machine_summary"]) == meta[0][1]
    plain = summarizer_amd.Summarizer(model, method="rank", max_ncp=10).summarize(torch.from_numpy(np.array(cases[0][0])).to(dev))
    assert plain["change_points"][-1, 1] == 64 and len(plain["machine_summary"]) == 65 and len(plain["change_points"]) <= 11
    with pytest.raises(TypeError):
        summarizer_amd.Summarizer(model, lmni=3)


# ------------------------------------------------------------------------------------------------ 7. Trainer opt-in
def _trainer(ds, keys, **over):
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.hps import make_hps
    hps = make_hps(ds, [{"train_keys": [], "test_keys": keys}], epochs=1, extra_params={"input_size": "128"}, **over)
    torch.manual_seed(77)
    return VASNetTrainer(hps, hps.splits_files[0]).reset()


def test_trainer_opt_in(dev):
    from summarizer_amd.utils.datasets import DictDataset, synthetic_dataset
    from summarizer_amd.utils.kts import cps_to_segments
    full = synthetic_dataset(4, seed=23, D=128, t_range=(40, 90), n_users=5)
    keys = sorted(full.keys(), key=lambda k: int(k.split("_")[1]))
    fields = lambda k, drop=(): {f: full[k][f][...] for f in full[k] if f not in drop}
    bare = DictDataset({k: fields(k, ("change_points", "n_frame_per_seg")) for k in keys})
    with pytest.raises(Exception, match="No /change_points in video video_1 for summary evaluation, make sure you have up-to-date .h5 dataset files."):
        _trainer(bare, keys).test(0)
    # the same dataset with the reference's segments written in by hand
    by_hand = {}
    for k in keys:
        rec = fields(k, ("change_points", "n_frame_per_seg"))
        X = rec["features"].astype(np.float64)
        n = X.shape[0]
        mb, cps, s, cost = kts_ref.cpd_auto(X @ X.T, min(n - 1, 1023), full=True)
        s32 = kts_ref.cpd_auto((rec["features"] @ rec["features"].T).astype(np.float64), min(n - 1, 1023), full=True)[2]
        fin = np.isfinite(s)
        gate = max(4 * float(np.abs(s32 - s)[fin].max()), 2 * ULP * float(np.abs(s[fin]).max()))
        assert kts_ref.cost_margin(cost) > 100 * gate / n, (k, kts_ref.cost_margin(cost), gate)
        rec["change_points"], rec["n_frame_per_seg"] = cps_to_segments(cps, rec["picks"], int(rec["n_frames"]))
        by_hand[k] = rec
    want = _trainer(DictDataset(by_hand), keys).test(0)
    tr = _trainer(bare, keys)
    tr.hps.change_points = "kts"
    got = tr.test(0)
    assert np.isfinite(got[0]) and np.isfinite(got[1][0]) and np.isfinite(got[1][1]) and got[1][1] > 0
    assert got == want, (got, want)
    for k in keys:
        assert np.array_equal(tr._video_meta(k, "summary").cps, by_hand[k]["change_points"])
    assert tr.test(0) == got                                             # cached in _video_meta: computed once
    # videos that carry the field keep theirs under the opt-in
    tr2 = _trainer(full, keys)
    before = tr2.test(0)
    tr3 = _trainer(full, keys)
    tr3.hps.change_points = "kts"
    assert tr3.test(0) == before
    assert np.array_equal(tr3._video_meta(keys[0], "summary").cps, full[keys[0]]["change_points"][...])
