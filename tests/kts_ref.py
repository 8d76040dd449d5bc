"""Float64 numpy reference of kernel temporal segmentation (KTS, Potapov et al. 2014) as include/sumk.h defines it for sumk_kts: a helper
of tests/test_kts_host.py (which pins it against brute force) and tests/test_gpu_kts.py, not a test.  Written from the definition:

  J[i, j] = sum_{t=i..j} K[t, t] - (1 / (j - i + 1)) sum_{s,t=i..j} K[s, t]     from the diagonal's cumulative sum and a 2-D prefix sum
  I[0, l] = J[0, l - 1] for lmin <= l < lmax (exclusive), 1e101 elsewhere
  I[k, l] = min_{max(k lmin, l - lmax) <= t < l} I[k - 1, t] + J[t, l - 1],   p[k, l] = the smallest minimising t
  cost[k] = I[k, n] / n + (vmax k / (2 n)) (ln(n / k) + 1),   m_best = the smallest minimising k
"""
import numpy as np

BIG = 1e101


def scatter(K):
    """J (n, n) float64; entries below the diagonal are 0."""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    K1 = np.concatenate([[0.0], np.cumsum(np.diag(K))])
    K2 = np.zeros((n + 1, n + 1))
    K2[1:, 1:] = np.cumsum(np.cumsum(K, 0), 1)
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    L = (j - i + 1).astype(np.float64)
    L[L <= 0] = 1
    J = (K1[j + 1] - K1[i]) - (K2[j + 1, j + 1] + K2[i, i] - K2[j + 1, i] - K2[i, j + 1]) / L
    J[j < i] = 0
    return J


def dp(K, m, lmin=1, lmax=100000):
    """(I (m + 1, n + 1), p (m + 1, n + 1)) of the dynamic programme."""
    n = K.shape[0]
    J = scatter(K)
    I = np.full((m + 1, n + 1), BIG)
    I[0, lmin:lmax] = J[0, lmin - 1:lmax - 1]
    p = np.zeros((m + 1, n + 1), dtype=np.int64)
    for k in range(1, m + 1):
        for l in range((k + 1) * lmin, n + 1):
            t0 = max(k * lmin, l - lmax)
            c = J[t0:l, l - 1] + I[k - 1, t0:l]
            a = int(np.argmin(c))                       # numpy's argmin returns the first minimum: the smallest t
            I[k, l], p[k, l] = c[a], a + t0
    return I, p


def backtrack(p, m, n):
    cps, cur = np.zeros(m, dtype=np.int64), n
    for k in range(m, 0, -1):
        cps[k - 1] = cur = p[k, cur]
    return cps


def _scores(I, n):
    s = I[:, n].copy()
    s[s > 1e99] = np.inf
    return s


def cpd_nonlin(K, m, lmin=1, lmax=100000):
    """(cps (m,), scores (m + 1,))"""
    n = K.shape[0]
    I, p = dp(K, m, lmin, lmax)
    return backtrack(p, m, n), _scores(I, n)


def costs(scores, n, vmax=1.0):
    m = len(scores) - 1
    k = np.arange(1, m + 1)
    pen = np.zeros(m + 1)
    pen[1:] = vmax * k / (2.0 * n) * (np.log(n / k) + 1)
    return scores / n + pen


def cpd_auto(K, max_ncp, vmax=1.0, lmin=1, lmax=100000, full=False):
    """(cps (m_best,), scores (m_best + 1,)); full=True: (m_best, cps, all scores (m + 1,), cost (m + 1,)).  max_ncp is cut to n - 1."""
    n = K.shape[0]
    m = min(max_ncp, n - 1)
    I, p = dp(K, m, lmin, lmax)
    s = _scores(I, n)
    cost = costs(s, n, vmax)
    mb = int(np.argmin(cost)) if np.isfinite(cost).any() else 0
    cps = backtrack(p, mb, n)
    return (mb, cps, s, cost) if full else (cps, s[:mb + 1])


def objective(K, cps):
    """sum of J over the segments the change points cut [0, n) into, float64."""
    J = scatter(K)
    b = np.concatenate([[0], np.asarray(cps, dtype=np.int64), [K.shape[0]]])
    return float(sum(J[b[q], b[q + 1] - 1] for q in range(len(b) - 1)))


def cost_margin(cost):
    """best-versus-second difference of the finite costs (inf when there is only one)."""
    c = np.sort(cost[np.isfinite(cost)])
    return float(c[1] - c[0]) if len(c) > 1 else np.inf


def planted_features(n, D, n_segs, sigma, seed):
    """Piecewise-constant means plus noise, rows L2-normalised, every segment >= 5 steps: (X (n, D) float32, boundaries)."""
    rng = np.random.default_rng(seed)
    while True:
        b = np.sort(rng.choice(np.arange(6, n - 5), n_segs - 1, replace=False)) if n_segs > 1 else np.array([], dtype=np.int64)
        if n_segs == 1 or np.min(np.diff(np.concatenate([[0], b, [n]]))) >= 5:
            break
    lab = np.searchsorted(b, np.arange(n), side="right")
    mu = rng.standard_normal((n_segs, D))
    X = (mu[lab] + sigma * rng.standard_normal((n, D))).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X, b
