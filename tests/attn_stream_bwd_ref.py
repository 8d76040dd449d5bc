"""Numpy specification of the training form of unmasked multi-head attention over a packed batch and of its backward
(csrc/attn_stream.hip: sumk_attn_stream_train; csrc/attn_stream_bwd.hip: sumk_attn_stream_backward).  TEST INFRASTRUCTURE ONLY.

Per video v and head h, with keep_ij = recipes.dropout_keep(seed, site, ((packed row i * n_heads + h) << 20) | j, p):

    s_ij  = scale q_i . k_j        alpha_ij = softmax_j(s_ij)        a~_ij = keep_ij ? alpha_ij / (1 - p) : 0
    ctx_i = sum_j a~_ij v_j
    dV_j  = sum_i a~_ij dctx_i
    dA_ij = keep_ij ? (dctx_i . v_j) / (1 - p) : 0                   delta_i = dctx_i . ctx_i   (= sum_j dA_ij alpha_ij)
    dS_ij = scale alpha_ij (dA_ij - delta_i)      dQ_i = sum_j dS_ij k_j      dK_j = sum_i dS_ij q_i

by the DENSE route: all logits of a row, the global row maximum, alpha divided by its sum, the masks applied with a select (never a
multiply: a dropped NaN is 0).  The float64 run uses plain matrix products.  The float32 run is the YARDSTICK of the GPU tests: each of the
products (the logits, ctx, dA, dV, dQ, dK) is ONE accumulator chain with k ascending, every product and every add rounded to float32, as
tests/attn_stream_ref._chain does.  It does not restate the kernels' recomputation of alpha from a saved statistic nor their two-pass
order: those are what the kernels must keep under the gate on their own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import recipes  # noqa: E402
from attn_stream_ref import _chain  # noqa: E402


def keep_mask(seed, site, p, row0, T, n_heads, h):
    """(T, T) bool: keep_ij of the video whose first packed row is row0, head h.  p == 0: all True."""
    if p <= 0.0:
        return np.ones((T, T), dtype=bool)
    wid = (np.arange(T, dtype=np.uint64) + np.uint64(row0)) * np.uint64(n_heads) + np.uint64(h)
    idx = (wid[:, None] << np.uint64(20)) | np.arange(T, dtype=np.uint64)[None, :]
    return recipes.dropout_keep(seed, site, idx, p)


def mha_train(Q, K, V, dctx, lens, n_heads, scale, p=0.0, seed=0, site=0, dtype=np.float64, row0=0):
    """Q, K, V, dctx: (sum(lens), D).  Returns a dict of `dtype` arrays: ctx, dq, dk, dv (n, D); delta, delta_alt (n, n_heads), the two forms
    of delta (dctx . ctx, and sum_j dA_ij alpha_ij).  row0: the packed row of the first row given (the tail of a longer batch)."""
    f = np.dtype(dtype).type
    chain = f is np.float32
    mm = (lambda a, b: _chain(np.ascontiguousarray(a), np.ascontiguousarray(b))) if chain else (lambda a, b: a @ b)
    Q, K, V, dctx = (np.asarray(a).astype(f) for a in (Q, K, V, dctx))
    n, D = Q.shape
    dh = D // n_heads
    sc = f(scale)
    ks = f(1.0) / (f(1.0) - f(np.float32(p)))
    zero = f(0.0)
    out = {k: np.zeros((n, D), dtype=f) for k in ("ctx", "dq", "dk", "dv")}
    out["delta"] = np.zeros((n, n_heads), dtype=f)
    out["delta_alt"] = np.zeros((n, n_heads), dtype=f)
    r0 = 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for T in lens:
            rows = slice(r0, r0 + T)
            for h in range(n_heads):
                cols = slice(h * dh, (h + 1) * dh)
                q, k, v, g = Q[rows, cols], K[rows, cols], V[rows, cols], dctx[rows, cols]
                keep = keep_mask(seed, site, p, row0 + r0, T, n_heads, h)
                e = mm(q, k.T) * sc
                m = e.max(axis=1, keepdims=True)                      # NaN in a row makes the whole row NaN (np.max propagates it)
                pe = np.exp(e - m)
                alpha = (pe / pe.sum(axis=1, keepdims=True, dtype=f)).astype(f)
                at = np.where(keep, alpha * ks, zero).astype(f) if p > 0.0 else alpha
                ctx = mm(at, v)
                dA = mm(g, v.T)
                if p > 0.0:
                    dA = np.where(keep, dA * ks, zero).astype(f)
                if chain:
                    delta = np.zeros(T, dtype=f)
                    for d in range(dh):
                        delta = delta + g[:, d] * ctx[:, d]
                else:
                    delta = (g * ctx).sum(axis=1)
                dS = (alpha * (dA - delta[:, None]) * sc).astype(f)
                out["ctx"][rows, cols] = ctx
                out["dv"][rows, cols] = mm(at.T, g)
                out["dq"][rows, cols] = mm(dS, k)
                out["dk"][rows, cols] = mm(dS.T, q)
                out["delta"][rows, h] = delta
                out["delta_alt"][rows, h] = (dA * alpha).sum(axis=1, dtype=f)
            r0 += T
    return out
