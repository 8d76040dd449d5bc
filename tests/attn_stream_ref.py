"""Numpy specification of unmasked multi-head attention over a packed batch (csrc/attn_stream.hip: sumk_attn_stream).  TEST INFRASTRUCTURE ONLY.

Per video v and head h:  ctx[rows of v, h dh : (h + 1) dh] = softmax_j(scale Q_h K_h^T) V_h  and  lse[rows of v, h] = log sum_j exp(scale q . k_j),
by the DENSE formula: all logits of a row, the global row maximum m, p_j = exp(fma(s_j, scale, -m)) (in numpy: s_j * scale - m, one more
rounding than the fused form), ctx = (p V) / sum p after dividing the weights by their sum as the dense kernel does, lse = m + log(sum p).
tests/test_attn_stream_host.py pins the float64 run of this file to oracle/transformer_np._mha's attention and to torch's
scaled_dot_product_attention.

The float32 run is the YARDSTICK of the GPU tests (the error float32 arithmetic costs on this problem), so its two products are summed the way
an exact-fp32 MFMA GEMM sums them: ONE accumulator per output element walking k in ascending order, every product and every add rounded to
float32 (`_chain`, the rule oracle/torch_port.mm_chain states for the library's fp32 GEMMs).  It is the dense order on purpose: it does not
restate the kernel's online rescale, which is the one thing the kernel must keep below the gate on its own.  The float64 run uses plain
matrix products: at float64 the order moves nothing above 1e-12."""
import numpy as np


def _chain(a, b):
    """a (M, K) @ b (K, N) with one accumulator per element, k ascending, in the operands' dtype."""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=a.dtype)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * b[None, k, :]
    return acc


def mha(Q, K, V, lens, n_heads, scale, dtype=np.float64):
    """Q, K, V: (sum(lens), D).  Returns (ctx (n, D), lse (n, n_heads)) in `dtype`."""
    f = np.dtype(dtype).type
    chain = f is np.float32
    Q, K, V = (np.asarray(a).astype(f) for a in (Q, K, V))
    n, D = Q.shape
    dh = D // n_heads
    sc = f(scale)
    ctx = np.zeros((n, D), dtype=f)
    lse = np.zeros((n, n_heads), dtype=f)
    r0 = 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for T in lens:
            rows = slice(r0, r0 + T)
            for h in range(n_heads):
                cols = slice(h * dh, (h + 1) * dh)
                q, k, v = Q[rows, cols], K[rows, cols], V[rows, cols]
                s = _chain(q, np.ascontiguousarray(k.T)) if chain else q @ k.T
                e = s * sc
                m = e.max(axis=1, keepdims=True)                      # NaN in a row makes the whole row NaN (np.max propagates it)
                p = np.exp(e - m)
                tot = p.sum(axis=1, keepdims=True, dtype=f)
                a = (p / tot).astype(f)
                ctx[rows, cols] = _chain(a, v) if chain else a @ v
                lse[rows, h] = (m + np.log(tot))[:, 0]
            r0 += T
    return ctx, lse
