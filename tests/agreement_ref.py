"""Plain numpy / scipy specification of the inter-annotator agreement (include/sumk.h: sumk_rank_rows, sumk_agreement_f,
sumk_agreement_corr; summarizer_amd/utils/agreement.py): how well the annotators of ONE video agree with each other under the two metrics
every model is measured by -- a helper module of the tests, in the role tests/annotate_ref.py plays for the dataset records.

F[a][b]    the reference's evaluate_summary(user_summary[a], user_summary[b:b+1])[0] (summarizer/utils/eval.py:125-165), one float32
           operation at a time: binarise with > 0, overlap, P = o / (sum_a + 1e-8), R = o / (sum_b + 1e-8), F = 2PR / (P + R), 0 when both
           are 0.  f_avg[a] / f_max[a]: float32 mean (numpy's pairwise tree) / maximum over b != a in index order; the video's values: the
           float64 mean of those over a.  NaN below two annotators.
rho[a][b]  Spearman: r = rankdata(-x), d = r - (n + 1) / 2, rho = (d_a . d_b) / sqrt(ssq_a ssq_b).  Every partial sum is a multiple of 0.25
           below 2^53 for n <= 16384: numerator and ssq are exact in any order.  A constant row: 0 / 0 = NaN, as scipy.
tau[a][b]  Kendall's tau-b from integer pair counts and the three float64 operations of kendall_tau_b (csrc/evaldev_common.h), x = a, y = b.
corr[a]    float64 mean over b != a, the video's corr the mean of those over a: numpy's pairwise order, NaN propagates; NaN below two."""
import warnings

import numpy as np
from scipy import stats

from annotate_ref import pairwise_sum

F32, F64 = np.float32, np.float64


def pairwise_sum64(a):
    """numpy's pairwise summation of at most 128 float64 values written out (np_pairwise_leaf of csrc/evaldev_common.h)."""
    a = np.asarray(a, dtype=F64)
    n = a.shape[0]
    assert n <= 128
    if n < 8:
        r = F64(0)
        for i in range(n):
            r = r + a[i]
        return F64(r)
    r = a[:8].copy()
    i = 8
    while i < n - (n % 8):
        r = r + a[i:i + 8]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + a[i]
        i += 1
    return F64(res)


def mean64(a):
    a = np.asarray(a, dtype=F64)
    with np.errstate(invalid="ignore"):
        return F64(pairwise_sum64(a) / F64(a.shape[0])) if a.shape[0] else F64(np.nan)


def f_pair(sa, sb):
    """float32 F-score of the 0 / 1 rows sa (in the machine's place) and sb (the annotator's)."""
    o = F32((sa * sb).sum(dtype=F32))                                # (sums of 0 / 1 values: exact in any order up to 2^24)
    p = F32(o / F32(F32(sa.sum(dtype=F32)) + F32(1e-8)))
    r = F32(o / F32(F32(sb.sum(dtype=F32)) + F32(1e-8)))
    if p == 0 and r == 0:
        return F32(0)
    return F32(F32(F32(F32(2) * p) * r) / F32(p + r))


def f_matrix(user_summary):
    s = (np.asarray(user_summary) > 0).astype(F32)
    U = s.shape[0]
    return np.array([[f_pair(s[a], s[b]) for b in range(U)] for a in range(U)], dtype=F32).reshape(U, U)


def f_agreement(user_summary):
    """{"F" (U, U) float32, "f_avg_user" / "f_max_user" (U,) float32, "f_avg" / "f_max" float64}."""
    F = f_matrix(user_summary)
    U = F.shape[0]
    if U < 2:
        nan = np.full(U, np.nan, F32)
        return {"F": F, "f_avg_user": nan, "f_max_user": nan.copy(), "f_avg": F64(np.nan), "f_max": F64(np.nan)}
    fa, fm = np.empty(U, F32), np.empty(U, F32)
    for a in range(U):
        others = np.delete(F[a], a)
        fa[a] = F32(pairwise_sum(others) / F32(U - 1))
        fm[a] = others.max()
    return {"F": F, "f_avg_user": fa, "f_max_user": fm, "f_avg": mean64(fa), "f_max": mean64(fm)}


def rank_rows(user_scores):
    """What sumk_rank_rows leaves per row: {"ranks" float64 = rankdata(-x), "dense" int32 0-based ascending with the score, "ties" int64
    tied pairs, "mean" float64, "ssq" float64}."""
    x = np.asarray(user_scores, dtype=F32)
    ranks = np.stack([stats.rankdata(-x[u].astype(F64)) for u in range(x.shape[0])]) if x.shape[0] else np.zeros(x.shape, F64)
    dense = np.empty(x.shape, np.int32)
    ties = np.zeros(x.shape[0], np.int64)
    for u in range(x.shape[0]):
        _, inv, cnt = np.unique(x[u] + F32(0), return_inverse=True, return_counts=True)      # (+ 0: -0.0 and 0.0 are one value)
        dense[u] = inv.reshape(-1)
        cnt = cnt.astype(np.int64)
        ties[u] = int((cnt * (cnt - 1) // 2).sum())
    n = x.shape[1]
    mean = np.full(x.shape[0], (n + 1) / 2, F64)
    d = ranks - mean[:, None]
    return {"ranks": ranks, "dense": dense, "ties": ties, "mean": mean, "ssq": (d * d).sum(axis=1)}


def spearman_matrix(user_scores):
    r = rank_rows(user_scores)
    d = r["ranks"] - r["mean"][:, None]
    U = d.shape[0]
    C = np.empty((U, U), F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(U):
            for b in range(U):
                C[a, b] = F64((d[a] * d[b]).sum()) / np.sqrt(r["ssq"][a] * r["ssq"][b])
    return C


def kendall_tau_b(cmd, tot, xtie, ytie):
    """kendall_tau_b of csrc/evaldev_common.h: the operations and their order as scipy.stats.kendalltau has them."""
    if xtie == tot or ytie == tot:
        return F64(np.nan)
    tau = F64(cmd) / np.sqrt(F64(tot - xtie)) / np.sqrt(F64(tot - ytie))
    return F64(min(1.0, max(-1.0, tau)))


def _pair_ties(key):
    _, cnt = np.unique(key, return_counts=True)
    cnt = cnt.astype(np.int64)
    return int((cnt * (cnt - 1) // 2).sum())


def inversions(y):
    """Pairs i < j with y[i] > y[j] of non-negative integers, one bit level at a time: such a pair shares the bits above its highest
    differing bit, where y[i] has a 1 and y[j] a 0 -- per level, a stable sort by the bits above and a running count of ones."""
    y = np.asarray(y, np.int64)
    if y.shape[0] < 2:
        return 0
    inv = 0
    for level in range(max(1, int(y.max()).bit_length()) - 1, -1, -1):
        prefix = y >> (level + 1)
        order = np.argsort(prefix, kind="stable")
        p, b = prefix[order], (y[order] >> level) & 1
        ones = np.cumsum(b) - b                                      # ones in front, over the whole array: non-decreasing
        base = np.maximum.accumulate(np.where(np.r_[True, p[1:] != p[:-1]], ones, 0))      # ... in front of the element's group
        inv += int(((ones - base) * (1 - b)).sum())
    return inv


def kendall_counts(dx, dy):
    """{cmd, xtie, ytie, ntie} of two dense-rank rows, as integers.  Discordant pairs = inversions of y in (x, y) order: pairs tied in
    x come sorted by y there, pairs tied in y are no inversion."""
    dx, dy = np.asarray(dx, np.int64), np.asarray(dy, np.int64)
    n = dx.shape[0]
    tot = n * (n - 1) // 2
    xtie, ytie, ntie = _pair_ties(dx), _pair_ties(dy), _pair_ties(dx * (1 << 20) + dy)
    dis = inversions(dy[np.lexsort((dy, dx))])
    return tot - xtie - ytie + ntie - 2 * dis, xtie, ytie, ntie


def kendall_matrix(user_scores):
    """(tau (U, U) float64, counts (U, U, 4) int64 {cmd, xtie, ytie, ntie})."""
    r = rank_rows(user_scores)
    U, n = r["dense"].shape
    tot = n * (n - 1) // 2
    tau, counts = np.empty((U, U), F64), np.zeros((U, U, 4), np.int64)
    for a in range(U):
        for b in range(a, U):
            cmd, xt, yt, nt = kendall_counts(r["dense"][a], r["dense"][b])
            counts[a, b] = (cmd, xt, yt, nt); counts[b, a] = (cmd, yt, xt, nt)
            tau[a, b] = kendall_tau_b(cmd, tot, xt, yt); tau[b, a] = kendall_tau_b(cmd, tot, yt, xt)
    return tau, counts


def corr_agreement(user_scores, metric="spearmanr"):
    """{"C" (U, U) float64, "corr_user" (U,) float64, "corr" float64[, "counts" (U, U, 4) int64 for Kendall]}."""
    out = {}
    if metric == "spearmanr":
        C = spearman_matrix(user_scores)
    elif metric == "kendalltau":
        C, out["counts"] = kendall_matrix(user_scores)
    else:
        raise KeyError(f"Unknown metric {metric}")
    U = C.shape[0]
    cu = np.array([mean64(np.delete(C[a], a)) if U >= 2 else np.nan for a in range(U)], dtype=F64)
    out.update(C=C, corr_user=cu, corr=mean64(cu) if U >= 2 else F64(np.nan))
    return out


def agreement(user_summary=None, user_scores=None, metric="spearmanr"):
    """One video: what `summarizer_amd.utils.agreement.human_agreement` returns for it."""
    out = {}
    if user_summary is not None:
        out.update(f_agreement(user_summary))
    if user_scores is not None:
        out.update(corr_agreement(user_scores, metric))
    return out


def scipy_matrix(user_scores, metric):
    """The pairwise correlations through scipy itself, as the reference's evaluate_scores calls it (eval.py:60-63)."""
    x = np.asarray(user_scores, dtype=F32)
    f = stats.kendalltau if metric == "kendalltau" else stats.spearmanr
    r = [stats.rankdata(-x[u]) for u in range(x.shape[0])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.array([[f(r[a], r[b])[0] for b in range(len(r))] for a in range(len(r))], dtype=F64).reshape(len(r), len(r))


def graded(n_users, n_frames, seed):
    """TVSum-shaped rows: grades 1 .. 5 per frame, rescaled to [0, 1] (five distinct values: heavy ties)."""
    rng = np.random.default_rng(seed)
    return ((rng.integers(1, 6, size=(n_users, n_frames)).astype(F32) - F32(1)) / F32(4)).astype(F32)


def continuous(n_users, n_frames, seed):
    """Rows that follow one hidden signal with noise: positive agreement, (almost) no ties."""
    rng = np.random.default_rng(seed)
    base = rng.random(n_frames)
    return (base[None, :] + 0.7 * rng.random((n_users, n_frames))).astype(F32)


def selections(n_users, n_frames, seed, density=0.3):
    """SumMe-shaped rows: 0 / positive marks (any value > 0 means selected)."""
    rng = np.random.default_rng(seed)
    return ((rng.random((n_users, n_frames)) < density) * rng.integers(1, 4, size=(n_users, n_frames))).astype(F32)
