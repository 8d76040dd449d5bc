"""Band-only numpy specification of the BACKWARD of local attention (csrc/attn_band_bwd.hip: sumk_attn_band_backward).  TEST INFRASTRUCTURE ONLY.

Forward, per video and per query row i over the keys j in [i - w, i + w] clipped to the video (tests/attn_band_ref.py):
    e = mask(q_i . k_j * scale),  alpha = softmax_j(e),  alphaD = alpha * keep,  ctx_i = sum_j alphaD_ij v_j.
Backward, given dCTX:
    dAlphaD_ij = dctx_i . v_j,  dAlpha = dAlphaD * keep,  dS_ij = scale * alpha_ij * (dAlpha_ij - sum_j' dAlpha_ij' alpha_ij'),
    dQ_i = sum_j dS_ij k_j,     dK_j = sum_i dS_ij q_i,   dV_j = sum_i alphaD_ij dctx_i      (i over the rows [j - w, j + w] that see key j).
Only keys [i - w, i + w] are touched: O(T w) work and memory, no (T x T) array.  `keep`: None, or already-scaled keep masks (0 or 1 / (1 - p))
in BAND LAYOUT, (rows x (2 w + 1)), column c of packed row r = key i - w + c of its video (columns of keys outside the video are ignored).
An all-masked row has NaN weights: its dQ is NaN and NaN reaches dK / dV at the keys of ITS band only (a key outside the video is no key;
a weight that dropout drops is 0, not NaN x 0: the kernels select, sumk::drop_apply).
tests/test_attn_band_bwd_host.py pins the float64 run to torch.autograd on the dense formula.

The float32 run is the YARDSTICK of the GPU tests.  Every matrix product of it -- the logits, dAlphaD, dQ, dK, dV -- is summed as ONE
accumulator per output element walking the contraction in ascending order, every product and every add rounded to float32
(attn_band_ref._chain: the project's rule for what an exact-fp32 MFMA GEMM can be held to).  The float64 run uses plain products."""
import numpy as np

from attn_band_ref import ROW_BLOCK, _chain


def _prod(a, b, chain):
    """sum_k a[n, k] * b[n, k, :] -> (n, N); chain: one ascending accumulator per element."""
    if chain:
        return _chain(a, np.ascontiguousarray(b.transpose(1, 0, 2)))
    return np.einsum("nk,nkd->nd", a, b)


def band_attention_backward(Q, K, V, dCTX, lens, w, scale, ignore_self=False, keep=None, dtype=np.float64, chain=None):
    """Q, K, V, dCTX: (sum(lens), D).  Returns (dQ, dK, dV), each (sum(lens), D) in `dtype`."""
    f = np.dtype(dtype).type
    chain = (f is np.float32) if chain is None else bool(chain)
    Q, K, V, dCTX = (np.asarray(a).astype(f) for a in (Q, K, V, dCTX))
    w = int(w)
    n_rows, D = Q.shape
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dQ, dK, dV = (np.zeros((n_rows, D), dtype=f) for _ in range(3))
    sc = f(scale)
    for v in range(len(lens)):
        r0, T = int(off[v]), int(off[v + 1] - off[v])
        we = min(w, T - 1)                                             # keys further than T - 1 away do not exist
        C = 2 * we + 1
        aD_all = np.zeros((T, C), dtype=f)                             # dropout(alpha) and dS of the video in band layout: O(T w)
        dS_all = np.zeros((T, C), dtype=f)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for b0 in range(0, T, ROW_BLOCK):
                i = np.arange(b0, min(T, b0 + ROW_BLOCK))
                J = i[:, None] - we + np.arange(C)[None, :]            # (n, C) key of every band column
                ok = (J >= 0) & (J < T)
                Jc = r0 + np.clip(J, 0, T - 1)
                q, dc = Q[r0 + i], dCTX[r0 + i]
                e = _prod(q, K[Jc].transpose(0, 2, 1), chain) * sc     # vasnet.py:118-119 on this block's band
                e[~ok] = -np.inf
                if ignore_self:
                    e[:, we] = -np.inf
                e[e * e == 0] = -np.inf                                # tril(e, w) * triu(e, -w) == 0 inside the band
                a = np.exp(e - e.max(axis=1, keepdims=True))
                a = (a / a.sum(axis=1, keepdims=True)).astype(f)
                a = np.where(ok, a, f(0))                              # a key outside the video is no key, even in a NaN row
                kp = np.ones((len(i), C), dtype=f) if keep is None else np.asarray(keep)[r0 + i, w - we:w - we + C].astype(f)
                aD = np.where(kp == 0, f(0), a * kp).astype(f)        # dropout SELECTS (sumk::drop_apply): a dropped weight is 0 even in a NaN row
                dA = np.where(kp == 0, f(0), _prod(dc, V[Jc].transpose(0, 2, 1), chain) * kp).astype(f)
                dot = (np.where(ok, dA, f(0)) * a).sum(axis=1, keepdims=True, dtype=f)
                dS = np.where(ok, a * (dA - dot) * sc, f(0)).astype(f)
                dQ[r0 + i] = _prod(dS, K[Jc], chain)
                aD_all[i], dS_all[i] = np.where(ok, aD, f(0)), dS
            for b0 in range(0, T, ROW_BLOCK):                          # keys: contract over the query rows [j - we, j + we], ascending
                j = np.arange(b0, min(T, b0 + ROW_BLOCK))
                I = j[:, None] - we + np.arange(C)[None, :]            # (n, C) query row of every band column
                ok = (I >= 0) & (I < T)
                Ic = np.clip(I, 0, T - 1)
                col = np.broadcast_to(2 * we - np.arange(C)[None, :], I.shape)      # key j stands at column j - i + we of row i
                aT = np.where(ok, aD_all[Ic, col], f(0))
                sT = np.where(ok, dS_all[Ic, col], f(0))
                dV[r0 + j] = _prod(aT, dCTX[r0 + Ic], chain)
                dK[r0 + j] = _prod(sT, Q[r0 + Ic], chain)
    return dQ, dK, dV
