"""GPU: DSN's training signal (csrc/reward.hip) against float64 -- sumk_dsn_reward (the Gram GEMM, reward_setup_kernel, reward_rows_kernel,
reward_final_kernel) against oracle/reward_np.reward_terms, sumk_dsn_policy_loss_forward / _backward (through autograd.PolicyLossFunction)
against oracle/policy_np.  tests/test_gpu_reward.py keeps its golden and at-size comparisons; what it cannot see is here: with
`recipes.features` R_rep = exp(-118) is 0 in fp32, so everything behind it (the min over picks, d2 = G[t][t] + G[p][p] - 2 G[t][p], / T, expf)
was compared with nothing.  `recipes.reward_features` scales the features so that 0.2 <= R_rep <= 1 in every case (tests/test_oracle.py
checks that on the oracle alone), which puts both terms of every compared reward five orders of magnitude above the gate.

Gates come from arithmetic, as in tests/test_gpu_optim.py: the float64 oracle is the reference, the SAME oracle run in fp32 on the CPU is the
yardstick (its distance to the float64 value), and the HIP value must stay within 4 x the yardstick, which has a floor of 2 fp32 ulps of the
value.  Reward: one scalar can land on the float64 value by chance, so the yardstick of a family is the LARGEST |fp32 oracle - float64
oracle| over the family's cases.  The term-isolating cases compare 2 r with R_rep (one pick) and 2 r - 1 or 2 r - R_rep with R_div (every
frame picked; two picks at the temporal threshold) under the same gate.  Policy loss: per case, the largest relative error of the loss per
video, and for the gradient the largest |error| / mag over ALL elements, mag = (|g0| + sum_e |adv_e (a - pc)| / (pc (1 - pc))) |scale| in
float64 (a gradient whose terms cancel is not judged by its own small value); elements with mag = 0 (an upstream gradient of exactly 0, or
beta = 0 outside the clamp) must be exactly 0.  No element is left out.  The policy inputs are well conditioned by construction
(recipes.policy_case says how and why) and the test asserts that on the float64 oracle.

The worst ratio (HIP error / yardstick) of every case is printed and kept in REPORT (written to $SUMK_REPORT_DIR when set).

Figures (yardstick = largest |fp32 oracle - float64 oracle| of the family, gate = 4 x yardstick, worst = largest HIP error /
yardstick over the family, 4 is the limit):
  NOT MEASURED: no MI355X run of this file exists yet, so no worst ratio is quoted.  What the CPU gives (the yardsticks are oracle against
  oracle, no kernel involved): tiles 4.27e-07 (gate 1.71e-06), isolation 1.12e-07 (4.49e-07), threshold 1.29e-07 (5.15e-07), many_videos
  2.38e-07 (9.54e-07), episodes 2.38e-07 (9.54e-07), zero_norm 1.43e-07 (5.72e-07); policy loss 2.0-7.8 ulp, gradient 2.8-5.6 ulp per case
  (gates 4 x).  With the fp32 oracle in place of the kernels every ratio is <= 2 (the doubled 2 r comparisons reach exactly 2).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import recipes as R
from oracle import policy_np, reward_np

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -24
REPORT = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for r in REPORT:
        print("REWARD-F64-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "reward_f64.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


# ------------------------------------------------------------------------------------------------ reward: references and the launch
def _oracle(calls):
    """[(terms64 (E, S, 3), reward32 (E, S))] per call and the yardstick: the largest |fp32 oracle - float64 oracle| over all of them.
    Calls that differ in far_sim only share their arrays; nothing here is modified afterwards."""
    refs, yard = [], 0.0
    for call in calls:
        off = np.concatenate([[0], np.cumsum(call["lens"])])
        E, S = call["acts"].shape[0], len(call["lens"])
        t64, r32 = np.zeros((E, S, 3)), np.zeros((E, S))
        for e in range(E):
            for s, x in enumerate(call["xs"]):
                a = call["acts"][e, off[s]:off[s + 1]]
                t64[e, s] = reward_np.reward_terms(x, a, call["far_sim"], call["thre"], np.float64)
                r32[e, s] = reward_np.compute_reward(x, a, call["far_sim"], call["thre"], np.float32)
        fin = np.isfinite(t64[:, :, 2])
        assert np.array_equal(fin, np.isfinite(r32))
        if fin.any():
            yard = max(yard, float(np.abs(r32 - t64[:, :, 2])[fin].max()))
        refs.append((t64, r32))
    return refs, yard


@functools.lru_cache(maxsize=None)
def _family(name):
    calls = R.reward_family(name)
    refs, yard = _oracle(calls)
    return calls, refs, yard


def _launch(dev, call):
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(call["lens"], dev)
    x = torch.from_numpy(np.concatenate(call["xs"])).to(dev)
    got = kernels.dsn_reward(x, sb, torch.from_numpy(call["acts"]).to(dev), far_sim=call["far_sim"], temp_dist_thre=call["thre"])
    assert got.shape == (call["acts"].shape[0], len(call["lens"])) and got.dtype == torch.float32
    return got.cpu().numpy()


def _compare(call, got, t64, yard):
    """Every (episode, video) of one call against the float64 terms.  Returns (worst error / yardstick, [failures])."""
    worst, bad = 0.0, []
    expect = call.get("expect", {})
    for e in range(got.shape[0]):
        for s in range(got.shape[1]):
            g = float(got[e, s])
            r_div, r_rep, ref = t64[e, s]
            what = expect.get((e, s))
            if what == "no_pick":                                    # dsn.py:199-203: exactly 0
                if g != 0.0:
                    bad.append((call["id"], e, s, what, g))
                continue
            y = max(yard, 2 * ULP * abs(ref))
            errs = {"reward": abs(g - ref)}
            if what == "one_pick":                                   # R_div = 0: twice the reward IS R_rep
                errs["2r_vs_r_rep"] = abs(2 * g - r_rep)
            elif what == "all_picked":                               # R_rep = exp(0) = 1: 2 r - 1 IS R_div
                errs["2r-1_vs_r_div"] = abs(2 * g - 1 - r_div)
            elif what in ("beyond_thre", "within_thre"):             # two picks: R_div is 1 beyond the threshold (unless far_sim), 1 - cos within it
                errs["2r-r_rep_vs_r_div"] = abs(2 * g - r_rep - r_div)
            for k, err in errs.items():
                worst = max(worst, err / y)
                if not err <= 4 * y:
                    bad.append((call["id"], e, s, what, k, g, ref, err, y))
    return worst, bad


def _check_family(dev, name, select=lambda call: True, tag=""):
    calls, refs, yard = _family(name)
    assert 0 < yard <= 1e-6, (name, yard)                            # (the recipe test on the CPU says the same)
    worst, bad, n = 0.0, [], 0
    for call, (t64, _) in zip(calls, refs):
        if not select(call):
            continue
        w, b = _compare(call, _launch(dev, call), t64, yard)
        worst, bad, n = max(worst, w), bad + b, n + 1
    assert n > 0
    REPORT.append(dict(family=name + tag, calls=n, yardstick=yard, gate=4 * yard, worst_ratio=worst))
    print("REWARD-F64", name + tag, "calls", n, "yardstick", yard, "gate", 4 * yard, "worst err/yardstick", round(worst, 3))
    assert not bad, (len(bad), bad[:8])


# ------------------------------------------------------------------------------------------------ reward: the families
@pytest.mark.parametrize("D", R.REWARD_TILE_D)
def test_reward_tile_and_padding_edges_vs_float64(dev, D):
    """One video per call: T in {1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 257, 320} (T % 4 != 0: the Gram row pitch (T + 3) & ~3; 64 k +- 1:
    the 64 x 64 Gram tiles), pick rates 0.05 / 0.4 / 1.0, both feature kinds, far_sim both ways; D = 36 and 100 leave a K tail."""
    _check_family(dev, "tiles", lambda call: call["D"] == D, tag=f"_D{D}")


def test_reward_terms_in_isolation_vs_float64(dev):
    """Exactly one pick (first, a middle, the last frame): R_div = 0, so 2 r is R_rep -- the min over picks, d2, / T and expf with nothing
    beside them.  Every frame picked: R_rep = 1, so 2 r - 1 is R_div."""
    _check_family(dev, "isolation")


def test_reward_temporal_threshold_boundary_vs_float64(dev):
    """Two picks exactly `thre` apart (R_div = 1 - cos) and `thre + 1` apart (R_div = 1 unless far_sim), thre in {0, 1, 20, T - 1, T + 5}
    at T = 70, at the start, in the middle and at the end of the video."""
    calls = _family("threshold")[0]
    for thre in (0, 1, 20, 69, 75):
        kinds = {c["expect"][(0, 0)] for c in calls if c["thre"] == thre}
        assert kinds == ({"beyond_thre"} if thre == 0 else {"within_thre"} if thre >= 69 else {"beyond_thre", "within_thre"}), (thre, kinds)
    _check_family(dev, "threshold")


@pytest.mark.parametrize("n_seq", [64, 65, 130])
def test_reward_many_videos_vs_float64(dev, n_seq):
    """More videos than one block of reward_setup_kernel takes (64): its second and third block, the offset binary search of
    reward_rows_kernel over 130 videos, one T = 129 video at position 70 among videos of 1..9 frames; three episodes."""
    calls = _family("many_videos")[0]
    assert any(len(c["lens"]) == 130 and c["lens"][70] == 129 and max(c["lens"][:70] + c["lens"][71:]) <= 9 for c in calls)
    _check_family(dev, "many_videos", lambda call: len(call["lens"]) == n_seq, tag=f"_n{n_seq}")


def test_reward_episodes_vs_float64(dev):
    """E = 1, 5, 9 episodes of the ragged batch [60, 1, 37, 130, 64] in one call: an episode without any pick (reward exactly 0 for every
    video, -0.0 actions included), one with one pick per video, one that picks everything, and action values 2.0 and -1.0 (picks)."""
    calls = _family("episodes")[0]
    assert {c["acts"].shape[0] for c in calls} == {1, 5, 9}
    a0 = calls[0]["acts"][0]
    assert (a0 == 2.0).any() and (a0 == -1.0).any() and np.signbit(a0[a0 == 0]).any() and not np.signbit(a0[a0 == 0]).all()
    _check_family(dev, "episodes")


def test_reward_workspace_reuse_gives_the_same_bits(dev):
    """The 130-video call, a one-video T = 5 call (which overwrites the head of the shared workspace: Gram, descriptors, row results),
    the 130-video call again: first and third result bit-identical."""
    big = next(c for c in _family("many_videos")[0] if c["id"] == "scaled_n130_far0")
    small = next(c for c in _family("tiles")[0] if c["id"] == "scaled_T5_D8_p0.4_far0")
    first, mid, third = _launch(dev, big), _launch(dev, small), _launch(dev, big)
    assert np.isfinite(first).all() and first.min() > 0.1 and mid.shape == (1, 1)
    assert np.array_equal(first.view(np.uint32), third.view(np.uint32))


def zero_norm_calls():
    """A batch whose middle video has one all-zero feature row (frame 17).  Episode 0 picks it among others, episode 1 leaves it out,
    episode 2 picks it alone (one pick: R_div = 0 by definition, no cosine is taken), episode 3 picks every frame."""
    lens, D, z = [9, 40, 5], 8, 17
    calls = []
    for kind in R.REWARD_KINDS:
        xs = [R.reward_features(kind, T, D, 5600 + i).copy() for i, T in enumerate(lens)]
        xs[1][z] = 0.0
        rng = np.random.default_rng(56)
        acts = (rng.random((4, sum(lens))) < 0.4).astype(np.float32)
        acts[:, [0, 9 + 3, 9 + 30, 9 + 40]] = 1.0                    # at least one pick per video, two besides frame 17 in the middle one
        acts[0, 9 + z], acts[1, 9 + z] = 1.0, 0.0
        acts[2, 9:9 + 40] = 0.0
        acts[2, 9 + z] = 1.0
        acts[3, :] = 1.0
        for far in (False, True):
            calls.append(dict(id=f"zero_norm_{kind}_far{int(far)}", lens=lens, D=D, xs=xs, acts=acts, far_sim=far, thre=5))
    return calls


def test_reward_zero_norm_frame_is_nan_where_the_oracle_says(dev):
    """A picked frame of zero norm among two picks or more: the cosine is 0 / 0, the float64 oracle (and the reference) give NaN.  The kernel
    must return NaN exactly there -- (episode 0, video 1) and (episode 3, video 1) -- and finite, correct values everywhere else."""
    calls = zero_norm_calls()
    refs, yard = _oracle(calls)
    want_nan = np.zeros((4, 3), bool)
    want_nan[0, 1] = want_nan[3, 1] = True
    worst, bad = 0.0, []
    for call, (t64, _) in zip(calls, refs):
        assert np.array_equal(np.isnan(t64[:, :, 2]), want_nan), call["id"]
        assert (t64[:, :, 1][~want_nan] >= 0.2).all(), (call["id"], t64[:, :, 1])        # R_rep is visible in the finite cases
        got = _launch(dev, call)
        assert np.array_equal(np.isnan(got), want_nan) and np.isfinite(got[~want_nan]).all(), (call["id"], got)
        keep = dict(call, expect={(e, s): "no_pick" for e in range(4) for s in range(3) if want_nan[e, s]})      # (skipped by _compare below)
        g = np.where(want_nan, 0.0, got)
        w, b = _compare(keep, g, np.where(want_nan[:, :, None], 0.0, t64), yard)
        worst, bad = max(worst, w), bad + b
    REPORT.append(dict(family="zero_norm", calls=len(calls), yardstick=yard, gate=4 * yard, worst_ratio=worst))
    print("REWARD-F64 zero_norm yardstick", yard, "worst err/yardstick", round(worst, 3))
    assert 0 < yard <= 1e-6 and not bad, (yard, bad[:8])


# ------------------------------------------------------------------------------------------------ REINFORCE policy loss
POLICY_E = (1, 15, 16, 17, 32, 33)                                    # across the PL_MAX_E = 16 register chunk of the forward kernel
POLICY_BETA = (0.0, 0.01, 1.0)
EPS_TARGET = 0.5


def _policy_hip(dev, c, beta):
    from summarizer_amd import kernels
    from summarizer_amd.autograd import PolicyLossFunction
    sb = kernels.SeqBatch.get(c["lens"], dev)
    t = lambda k: torch.from_numpy(c[k]).to(dev)
    p = t("probs").requires_grad_(True)
    lv = PolicyLossFunction.apply(p, sb, t("actions"), t("rewards"), t("base"), beta, EPS_TARGET)
    (lv * t("dlv")).sum().backward()
    return lv.detach().cpu().numpy().astype(np.float64), p.grad.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("E", POLICY_E)
@pytest.mark.parametrize("batch", R.POLICY_BATCHES)
def test_policy_loss_and_gradient_vs_float64(dev, batch, E):
    """"ragged": T = 1, 255, 256, 257, 513, 1100 -- the kernels step over the frames with t += 256, so one to five passes; "short": 70 videos
    of 1..9 frames.  beta = 0, 0.01, 1; advantages of both signs; an upstream gradient with both signs and exact zeros; probabilities 0, 1,
    eps and 1 - eps (on the closed clamp range: the log-prob gradient passes), one ulp outside either end, 1e-9, and ordinary values."""
    c = R.policy_case(batch, E)
    lens, off = np.asarray(c["lens"]), np.concatenate([[0], np.cumsum(c["lens"])])
    vid = np.repeat(np.arange(len(lens)), lens)
    pr = c["probs"]
    clamp = R.POLICY_CLAMP
    for v in (0.0, 1.0, clamp, np.float32(1) - clamp, np.float32(1e-9), np.nextafter(clamp, np.float32(0))):
        assert (pr == np.float32(v)).any(), v
    assert c["outside"].size >= 5 and (c["dlv"] == 0).any() and (c["dlv"] > 0).any() and (c["dlv"] < 0).any()
    adv = c["rewards"].astype(np.float64) - c["base"].astype(np.float64)[None, :]
    assert (adv > 0).any() and (adv < 0).any()
    mp = np.array([pr[off[v]:off[v + 1]].astype(np.float64).mean() for v in range(len(lens))])
    assert np.abs(mp - EPS_TARGET).min() >= 0.2                       # the penalty's gradient keeps a fifth of its operands' size
    bad = []
    for beta in POLICY_BETA:
        args = (pr, c["lens"], c["actions"], c["rewards"], c["base"], beta, EPS_TARGET)
        l64, cond = policy_np.forward(*args, np.float64)
        l32, _ = policy_np.forward(*args, np.float32)
        g64, mag = policy_np.backward(*args, c["dlv"], np.float64)
        g32, _ = policy_np.backward(*args, c["dlv"], np.float32)
        assert cond.max() <= 8, (beta, cond.max())                    # no video's loss is a cancellation of its terms
        lv, gp = _policy_hip(dev, c, beta)
        assert np.isfinite(lv).all() and np.isfinite(gp).all()
        # loss per video: relative error
        yl = max(float(np.max(np.abs(l32 - l64) / np.abs(l64))), 2 * ULP)
        el = float(np.max(np.abs(lv - l64) / np.abs(l64)))
        # gradient: error relative to the size of the element's terms; mag = 0 means the exact value is 0
        live = mag > 0
        assert (c["dlv"][vid] == 0)[~live].all() or beta == 0
        exact0 = bool((gp[~live] == 0).all()) and bool((gp[c["dlv"][vid] == 0] == 0).all())
        yg = max(float(np.max(np.abs(g32 - g64)[live] / mag[live])), 2 * ULP)
        eg = float(np.max(np.abs(gp - g64)[live] / mag[live]))
        # outside the clamp: the closed form w_v 2 beta (mean p - eps) / (E T_v), nothing else
        out = c["outside"]
        want = c["dlv"].astype(np.float64)[vid[out]] * 2 * beta * (mp[vid[out]] - EPS_TARGET) / (E * lens[vid[out]])
        np.testing.assert_allclose(g64[out], want, rtol=1e-12, atol=0)
        nz = want != 0
        ec = float(np.max(np.abs(gp[out] - want)[nz] / np.abs(want)[nz])) if nz.any() else 0.0
        closed0 = bool((gp[out][~nz] == 0).all())
        REPORT.append(dict(family="policy", batch=batch, E=E, beta=beta, loss_yardstick=yl, grad_yardstick=yg,
                           worst_ratio=dict(loss=el / yl, grad=eg / yg, outside_clamp=ec / yg)))
        print("REWARD-F64 policy", batch, "E", E, "beta", beta, "yardsticks (ulp) loss", round(yl / ULP, 2), "grad", round(yg / ULP, 2),
              "worst err/yardstick loss", round(el / yl, 3), "grad", round(eg / yg, 3), "outside the clamp", round(ec / yg, 3))
        if not (el <= 4 * yl and eg <= 4 * yg and ec <= 4 * yg and exact0 and closed0):
            bad.append((beta, el, yl, eg, yg, ec, exact0, closed0))
    assert not bad, bad
