"""Band-only numpy specification of local attention (csrc/attn_band.hip: sumk_attn_band).  TEST INFRASTRUCTURE ONLY.

Per video of a packed batch and per query row i, only the keys [i - w, i + w] clipped to the video are touched: O(T w) work and memory, no
(T x T) array.  The mask is `oracle.vasnet_np.attention_mask` restricted to the band: ignore_self puts -inf on the diagonal, and with
scope = tril(e, w) * triu(e, -w) every entry with scope == 0 is -inf -- inside the band scope = e * e, so an in-band logit whose square is
zero (or underflows to zero in `dtype`) is masked too.  A row with every key masked is NaN, as the dense oracle's (and torch's) softmax gives.
tests/test_attn_band_host.py pins the float64 run of this file to the dense oracle.

The float32 run is the YARDSTICK of the GPU tests (the error float32 arithmetic costs on this problem), so its two products are summed the
way an exact-fp32 MFMA GEMM sums them: ONE accumulator per output element walking k in ascending order, every product and every add
rounded to float32 (`chain=True`, the default for float32).  This is the rule `oracle/torch_port.mm_chain` states for the library's fp32
GEMMs: a BLAS product sums in blocks and lanes, its rounding error grows far slower with the length of the contraction than a chain's, and
is not what such a GEMM can be held to (csrc/gemm_f32.hip: "the sum over k is re-associated relative to a sequential loop").  The float64
run uses plain matrix products: at float64 the order moves nothing above 1e-12."""
import numpy as np

ROW_BLOCK = 64


def _chain(a, b):
    """sum_k a[..., k, None-or-:] * b[..., k, :] with one accumulator per element, k ascending, in the operands' dtype.
    a: (n, K) weights, b: (K, n, N) -> (n, N)."""
    acc = np.zeros((b.shape[1], b.shape[2]), dtype=b.dtype)
    for k in range(b.shape[0]):
        acc = acc + a[:, k, None] * b[k]
    return acc


def band_attention(Q, K, V, lens, w, scale, ignore_self=False, dtype=np.float64, rows=None, chain=None):
    """Q, K, V: (sum(lens), D).  Returns (ctx (n, D), alpha (n, 2 w + 1)) in `dtype`, one line per packed row -- or per entry of `rows`
    (packed row indices, any order) when given.  alpha[., c] is the weight of key i - w + c; keys outside the video get 0.
    chain: sum both products as one accumulator chain (module docstring); None = only when dtype is float32."""
    f = np.dtype(dtype).type
    chain = (f is np.float32) if chain is None else bool(chain)
    Q, K, V = (np.asarray(a) for a in (Q, K, V))
    w = int(w)
    D = Q.shape[1]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    todo = np.arange(off[-1]) if rows is None else np.asarray(rows, dtype=np.int64)
    ctx = np.zeros((len(todo), D), dtype=f)
    alpha = np.zeros((len(todo), 2 * w + 1), dtype=f)
    sc = f(scale)
    vid = np.searchsorted(off, todo, side="right") - 1
    for v in np.unique(vid):
        r0, T = int(off[v]), int(off[v + 1] - off[v])
        we = min(w, T - 1)                                         # keys further than T - 1 away do not exist
        C = 2 * we + 1
        sel = np.nonzero(vid == v)[0]
        for b0 in range(0, len(sel), ROW_BLOCK):
            out = sel[b0:b0 + ROW_BLOCK]
            i = todo[out] - r0                                     # rows inside the video
            J = i[:, None] - we + np.arange(C)[None, :]            # (n, C) key of every band column
            ok = (J >= 0) & (J < T)
            Jc = r0 + np.clip(J, 0, T - 1)
            q = Q[todo[out]].astype(f)
            if chain:
                e = _chain(q, np.ascontiguousarray(K[Jc].astype(f).transpose(2, 0, 1))) * sc      # vasnet.py:118-119, this block's band
            else:
                e = np.einsum("nck,nk->nc", K[Jc].astype(f), q) * sc
            e[~ok] = -np.inf
            if ignore_self:
                e[:, we] = -np.inf                                 # vasnet.py:121-122
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                e[e * e == 0] = -np.inf                            # vasnet.py:126-127 inside the band: tril(e, w) * triu(e, -w) = e * e
                m = e.max(axis=1, keepdims=True)
                a = np.exp(e - m)
                a = (a / a.sum(axis=1, keepdims=True)).astype(f)   # vasnet.py:129
                Vb = V[Jc].astype(f)
                if chain:
                    c = _chain(a, np.ascontiguousarray(Vb.transpose(1, 0, 2)))                    # vasnet.py:131
                else:
                    c = np.einsum("nc,ncd->nd", a, Vb)
            ctx[out] = c
            alpha[out, w - we:w - we + C] = np.where(ok, a, 0)     # keys outside the video carry 0 even in an all-masked (NaN) row
    return ctx, alpha
