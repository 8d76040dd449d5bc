"""numpy restatement of the REINFORCE loss glue of DSNTrainer.train (reference: summarizer/models/dsn.py:113-140) for a packed batch of
videos, in any dtype.  TEST INFRASTRUCTURE ONLY.

Per video v of T_v frames, with E episodes of actions a[e, t], rewards r[e, v], a baseline b[v] and the frame probabilities p_t:

    l_v = [ beta (mean_t p_t - eps)^2  -  sum_e (r[e, v] - b[v]) mean_t log P(a[e, t] | pc_t) ] / E
    log P(a | pc) = a log(pc) + (1 - a) log1p(-pc),    pc = clamp(p, c, 1 - c)

which is torch.distributions.Bernoulli(probs=p).log_prob(a) written out (probs_to_logits clamps the probabilities, then
binary_cross_entropy_with_logits).  c is torch.finfo(float32).eps in EVERY dtype: the reference runs in fp32 and the HIP kernels mirror
that program, so the float64 run of this file is the fp32 program's formula in exact arithmetic, not a float64 program with its own clamp.
1 - c is representable in fp32, so both dtypes clamp to the same two numbers.

Gradient with respect to p (rewards and baselines are constants of the step), for an upstream gradient w_v = dL / dl_v:

    dL/dp_t = w_v [ 2 beta (mean p - eps)  -  [c <= p_t <= 1 - c] sum_e (r - b)[e, v] (a[e, t] - pc_t) / (pc_t (1 - pc_t)) ] / (E T_v)

torch.clamp passes the gradient on its CLOSED range and blocks it outside, so a probability outside [c, 1 - c] keeps the length-penalty
term only.  tests/test_oracle.py pins both functions to Bernoulli.log_prob + autograd in float64."""
import numpy as np

CLAMP = float(np.finfo(np.float32).eps)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])


def forward(probs, lens, actions, rewards, base, beta, eps_target, dtype=np.float64):
    """probs (R,), actions (E, R), rewards (E, V), base (V,) -> (loss per video (V,), cond (V,)), both `dtype`.
    cond = (sum of the absolute values of the terms of l_v) / |l_v|: how much of its terms' rounding a video's loss shows."""
    f = dtype
    p, a = np.asarray(probs).astype(f), np.asarray(actions).astype(f)
    r, b = np.asarray(rewards).astype(f), np.asarray(base).astype(f)
    E, off = a.shape[0], _offsets(lens)
    pc = np.clip(p, f(CLAMP), f(1.0) - f(CLAMP))
    logp = a * np.log(pc)[None, :] + (f(1.0) - a) * np.log1p(-pc)[None, :]                 # (E, R)
    lv, cond = np.zeros(len(lens), f), np.zeros(len(lens), f)
    for v in range(len(lens)):
        s = slice(off[v], off[v + 1])
        pen = f(beta) * (p[s].mean(dtype=f) - f(eps_target)) ** 2
        terms = (r[:, v] - b[v]) * logp[:, s].mean(axis=1, dtype=f)                       # (E,)
        lv[v] = (pen - terms.sum(dtype=f)) / f(E)
        cond[v] = (abs(pen) + np.abs(terms).sum(dtype=f)) / f(E) / max(abs(lv[v]), np.finfo(f).tiny)
    return lv, cond


def backward(probs, lens, actions, rewards, base, beta, eps_target, dlv, dtype=np.float64):
    """-> (dprobs (R,), mag (R,)), both `dtype`.  mag is the sum of the absolute values of an element's terms,
    (|g0| + [inside] sum_e |adv_e (a - pc)| / (pc (1 - pc))) |w_v| / (E T_v): the size against which the element's rounding error is
    judged (the terms of a gradient may cancel)."""
    f = dtype
    p, a = np.asarray(probs).astype(f), np.asarray(actions).astype(f)
    r, b, w = np.asarray(rewards).astype(f), np.asarray(base).astype(f), np.asarray(dlv).astype(f)
    E, off = a.shape[0], _offsets(lens)
    lo, hi = f(CLAMP), f(1.0) - f(CLAMP)
    pc = np.clip(p, lo, hi)
    inside = (p >= lo) & (p <= hi)
    inv = f(1.0) / (pc * (f(1.0) - pc))
    dp, mag = np.zeros_like(p), np.zeros_like(p)
    for v in range(len(lens)):
        s = slice(off[v], off[v + 1])
        T = off[v + 1] - off[v]
        adv = (r[:, v] - b[v])[:, None]                                                    # (E, 1)
        scale = w[v] / (f(E) * f(T))
        g0 = f(2.0) * f(beta) * (p[s].mean(dtype=f) - f(eps_target))
        t = adv * (a[:, s] - pc[s][None, :])                                               # (E, T)
        dp[s] = (g0 - np.where(inside[s], t.sum(axis=0, dtype=f) * inv[s], f(0.0))) * scale
        mag[s] = (abs(g0) + np.where(inside[s], np.abs(t).sum(axis=0, dtype=f) * inv[s], f(0.0))) * abs(scale)
    return dp, mag
