"""Float64 numpy specification of BANDED kernel temporal segmentation (sumk_kts_banded, include/sumk.h): the definition of tests/kts_ref.py
with only the band J[t, t .. t + B - 1], B = min(lmax, n), ever held -- O(n B) memory, so it reaches the lengths the (n x n) reference
cannot.  A helper of tests/test_kts_banded_host.py (which pins it against kts_ref) and tests/test_gpu_kts_banded.py, not a test.

  band of K   Kc[j, d] = K[j - d, j]  (d = 0 .. B - 1), from a full matrix (`band_from_gram`) or from features in row blocks (`band_from_features`)
  W           Wc[j, d] = K[j, j] + sum_{1 <= d' <= d} 2 K[j - d', j]        cumulative sum along d: the increment S(j - d, j) - S(j - d, j - 1) of
                                                                            the block sum S(i, j) = sum_{s,t=i..j} K[s, t] of a SYMMETRIC K
  J band      Jb[i, c] = sum_{t=i..i+c} K[t, t] - S(i, i + c) / (c + 1),  S(i, i + c) = sum_{c' <= c} Wc[i + c', c']   cumulative sum along the row
  DP          I[0, l] = Jb[0, l - 1] (lmin <= l < lmax, exclusive), 1e101 elsewhere;
              I[k, l] = min_{max(k lmin, l - lmax) <= t < l} I[k - 1, t] + Jb[t, l - 1 - t],  p[k, l] = the smallest minimising t
Both cumulative sums start at the segment's own corner (no cancellation of n^2-sized prefix sums).  Entries of the band past the video's
end are 0 and never read."""
import numpy as np

import kts_ref

BIG = kts_ref.BIG


def band_width(n, lmax):
    return int(min(lmax, n))


def band_from_gram(K, B):
    """Kc (n, B): Kc[j, d] = K[j - d, j], 0 where j - d < 0."""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    j, d = np.arange(n)[:, None], np.arange(B)[None, :]
    return np.where(j - d >= 0, K[np.maximum(j - d, 0), j], 0.0)


def band_from_features(X, B, dtype=np.float64, block=2048):
    """The same band of K = X X^T without the (n x n) matrix: row blocks of `block` columns j against the B + block - 1 rows they reach.
    dtype=float32 computes the products in float32 (numpy's matmul), the yardstick of the fp32-Gram tests."""
    X = np.ascontiguousarray(X, dtype=dtype)
    n = X.shape[0]
    Kc = np.zeros((n, B), dtype=np.float64)
    d = np.arange(B)[None, :]
    for j0 in range(0, n, block):
        j1 = min(n, j0 + block)
        s0 = max(0, j0 - B + 1)
        P = (X[j0:j1] @ X[s0:j1].T).astype(np.float64)            # P[j - j0, s - s0]
        j = np.arange(j0, j1)[:, None]
        s = j - d
        Kc[j0:j1] = np.where(s >= 0, P[j - j0, np.maximum(s, 0) - s0], 0.0)
    return Kc


def scatter_band(Kc):
    """Jb (n, B) float64 from the band Kc of a symmetric K: Jb[i, c] = J[i, i + c]; 0 where i + c >= n."""
    n, B = Kc.shape
    Wc = Kc.copy()
    Wc[:, 1:] *= 2.0
    Wc = np.cumsum(Wc, axis=1)                                    # Wc[j, d] = W[j - d][j]
    i, c = np.arange(n)[:, None], np.arange(B)[None, :]
    ok = i + c < n
    t = np.minimum(i + c, n - 1)
    S = np.cumsum(np.where(ok, Wc[t, c], 0.0), axis=1)            # S(i, i + c)
    Dg = np.cumsum(np.where(ok, Kc[t, 0], 0.0), axis=1)           # sum of the diagonal over i .. i + c
    return np.where(ok, Dg - S / (c + 1.0), 0.0)


def dp_band(Jb, m, lmin=1, lmax=100000):
    """(I (m + 1, n + 1), p (m + 1, n + 1)) of the dynamic programme on the band; O(n B) work per row, vectorised over (l, l - 1 - t)."""
    n, B = Jb.shape
    lmax_c = int(min(lmax, n + 1))
    I = np.full((m + 1, n + 1), BIG)
    if lmin < lmax_c:
        I[0, lmin:lmax_c] = Jb[0, lmin - 1:lmax_c - 1]
    p = np.zeros((m + 1, n + 1), dtype=np.int64)
    if m == 0:
        return I, p
    # JlR[l, e] = Jb[t, l - 1 - t] at t = l - B + e: the scatter of the segment t .. l - 1, the columns in ASCENDING t (inf where t < 0)
    l, e = np.arange(n + 1)[:, None], np.arange(B)[None, :]
    t = l - B + e
    JlR = np.where(t >= 0, Jb[np.maximum(t, 0), np.maximum(l - 1 - t, 0)], np.inf)
    c = np.empty_like(JlR)
    for k in range(1, m + 1):
        lo = (k + 1) * lmin
        if lo > n:
            break
        prev = np.concatenate([np.full(B, np.inf), I[k - 1]])
        prev[:B + k * lmin] = np.inf                              # t >= k lmin (t >= l - lmax is the band itself)
        win = np.lib.stride_tricks.sliding_window_view(prev, B)[lo:n + 1]                     # win[l - lo, e] = I[k - 1, l - B + e]
        np.add(JlR[lo:], win, out=c[lo:])
        a = np.argmin(c[lo:], axis=1)                             # the first minimum along ascending t: the smallest t at a tie
        I[k, lo:] = c[lo:][np.arange(n + 1 - lo), a]
        p[k, lo:] = np.arange(lo, n + 1) - B + a
    return I, p


def _finish(I, p, n, m, vmax, full):
    s = kts_ref._scores(I, n)
    cost = kts_ref.costs(s, n, vmax)
    mb = int(np.argmin(cost)) if np.isfinite(cost).any() else 0
    cps = kts_ref.backtrack(p, mb, n)
    return (mb, cps, s, cost) if full else (cps, s[:mb + 1])


def cpd_nonlin_band(Kc, m, lmin=1, lmax=100000):
    """(cps (m,), scores (m + 1,)) from the band of K."""
    n = Kc.shape[0]
    I, p = dp_band(scatter_band(Kc), m, lmin, lmax)
    return kts_ref.backtrack(p, m, n), kts_ref._scores(I, n)


def cpd_auto_band(Kc, max_ncp, vmax=1.0, lmin=1, lmax=100000, full=False):
    """kts_ref.cpd_auto from the band of K (Kc must be band_width(n, lmax) wide)."""
    n = Kc.shape[0]
    assert Kc.shape[1] == band_width(n, lmax), (Kc.shape, lmax)
    m = min(max_ncp, n - 1)
    I, p = dp_band(scatter_band(Kc), m, lmin, lmax)
    return _finish(I, p, n, m, vmax, full)


def cpd_auto(K, max_ncp, vmax=1.0, lmin=1, lmax=100000, full=False):
    """The same from a full symmetric (n x n) matrix: the signature of kts_ref.cpd_auto."""
    K = np.asarray(K, dtype=np.float64)
    return cpd_auto_band(band_from_gram(K, band_width(K.shape[0], lmax)), max_ncp, vmax, lmin, lmax, full)


def cpd_auto_features(X, max_ncp, vmax=1.0, lmin=1, lmax=100000, full=False, dtype=np.float64):
    """The same from features (K = X X^T), never forming K."""
    return cpd_auto_band(band_from_features(X, band_width(X.shape[0], lmax), dtype), max_ncp, vmax, lmin, lmax, full)
