"""Numpy specification of the bf16x3 training form of the streaming attention and of its backward (csrc/attn_stream_split.hip:
sumk_attn_stream_split_train; csrc/attn_stream_split_bwd.hip: sumk_attn_stream_split_backward).  TEST INFRASTRUCTURE ONLY.

The dense formula of tests/attn_stream_bwd_ref.py in float32 with the roundings of the bf16x3 arithmetic (tests/attn_stream_split_ref.py:
split, chain3 -- every operand two bf16 planes, a product hi.hi + hi.lo + lo.hi in one float32 accumulator per element, k ascending):

    s = q3.k3;  m = max_j s_j scale;  pe_j = exp(s_j scale - m);  l = sum_j pe_j                      (float32)
    p~ = keep ? pe / (1 - p) : 0, split;  O = p~3.v3;  ctx = O / l                                     (the forward)
    alpha = pe (1 / l);  a~ = keep ? alpha / (1 - p) : 0;  dA = g3.v3^T, masked by a select and rescaled
    delta = g . ctx, ONE float32 chain over the head's columns (the fp32 launch)
    dS = alpha (dA - delta) scale in float32;  a~, dS and their transposes split
    dV = a~^T3.g3;  dQ = dS3.k3;  dK = dS^T3.q3

All six matrix products go through chain3.  This is the YARDSTICK of the GPU tests: what the arithmetic costs on a problem.  The REFERENCE
stays attn_stream_bwd_ref.mha_train in float64 on the unsplit inputs.  `acc=np.float64` sums the same plane products in float64
(tests/test_attn_stream_split_bwd_host.py holds that run to oracle/torch_port.mm3).

`mutant` builds the wrong kernels the gate has to catch (tests/test_attn_stream_split_bwd_host.py):
  "da_no_lohi"       lo.hi dropped in dA                         "ds_one_plane"     dS as one bf16 plane (dQ and dK)
  "at_one_plane"     a~ as one bf16 plane in dV                  "da_no_mask"       the mask not applied to dA (the rescale neither)
  "mask_permuted"    the backward's masks drawn at the position a key has in the transposed planes (bits 2 and 3 of the key swapped)
                     instead of at the true key
  "drop_last_walked" the last query of a partial last tile lost in dK and dV
  "delta_neighbour"  delta taken from head h + 1 (mod n_heads)"""
import numpy as np

from attn_stream_bwd_ref import keep_mask
from attn_stream_split_ref import KEY_TILE, chain3, split

MUTANTS = ("da_no_lohi", "ds_one_plane", "at_one_plane", "da_no_mask", "mask_permuted", "drop_last_walked", "delta_neighbour")


def _perm(j):
    """position <-> row inside a 64-row tile of a transposed plane: bits 2 and 3 swapped."""
    return (j & ~12) | ((j & 8) >> 1) | ((j & 4) << 1)


def _split_or_one(x, one_plane):
    hi, lo = split(x)
    return (hi, np.zeros_like(lo)) if one_plane else (hi, lo)


def mha3_train(Q, K, V, dctx, lens, n_heads, scale, p=0.0, seed=0, site=0, acc=np.float32, mutant=None, row0=0):
    """Q, K, V, dctx: (sum(lens), D) float32.  Returns a dict of float32 arrays: ctx, dq, dk, dv (n, D); delta (n, n_heads).
    row0: the packed row of the first row given (the tail of a longer batch)."""
    assert mutant is None or mutant in MUTANTS, mutant
    f = np.float32
    Q, K, V, dctx = (np.asarray(a, dtype=f) for a in (Q, K, V, dctx))
    n, D = Q.shape
    dh = D // n_heads
    sc = f(scale)
    ks = f(1.0) / (f(1.0) - f(p))
    zero = f(0.0)
    T_ = lambda a: np.ascontiguousarray(a.T)
    out = {k: np.zeros((n, D), dtype=f) for k in ("ctx", "dq", "dk", "dv")}
    out["delta"] = np.zeros((n, n_heads), dtype=f)
    r0 = 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for T in lens:
            rows = slice(r0, r0 + T)
            fwd = []
            for h in range(n_heads):                                       # the forward and delta of every head (a mutant crosses heads)
                cols = slice(h * dh, (h + 1) * dh)
                q, k, v, g = Q[rows, cols], K[rows, cols], V[rows, cols], dctx[rows, cols]
                keep = keep_mask(seed, site, p, row0 + r0, T, n_heads, h)
                s = chain3(q, T_(k), acc).astype(f)
                e = s * sc
                m = e.max(axis=1, keepdims=True)
                pe = np.exp(e - m).astype(f)
                tot = pe.sum(axis=1, keepdims=True, dtype=f)
                pd = np.where(keep, pe * ks, zero).astype(f) if p > 0.0 else pe
                ctx = (chain3(split(pd), v, acc).astype(f) / tot).astype(f)
                delta = np.zeros(T, dtype=f)
                for d in range(dh):
                    delta = delta + g[:, d] * ctx[:, d]
                out["ctx"][rows, cols] = ctx
                out["delta"][rows, h] = delta
                fwd.append((pe, tot, keep))
            for h in range(n_heads):
                cols = slice(h * dh, (h + 1) * dh)
                q, k, v, g = Q[rows, cols], K[rows, cols], V[rows, cols], dctx[rows, cols]
                pe, tot, keep = fwd[h]
                if mutant == "mask_permuted" and p > 0.0:
                    j = np.arange(T)
                    pj = (j & ~63) | _perm(j & 63)
                    keep = keep[:, np.where(pj < T, pj, j)]
                delta = out["delta"][rows, (h + 1) % n_heads if mutant == "delta_neighbour" else h]
                alpha = (pe * (f(1.0) / tot)).astype(f)
                at = np.where(keep, alpha * ks, zero).astype(f) if p > 0.0 else alpha
                dA = chain3(g, T_(v), acc, (True, True, mutant != "da_no_lohi")).astype(f)
                if p > 0.0 and mutant != "da_no_mask":
                    dA = np.where(keep, dA * ks, zero).astype(f)
                dS = (alpha * (dA - delta[:, None]) * sc).astype(f)
                one = mutant == "ds_one_plane"
                out["dq"][rows, cols] = chain3(_split_or_one(dS, one), k, acc).astype(f)
                atw, dSw = at, dS
                if mutant == "drop_last_walked" and T % KEY_TILE:
                    atw, dSw = at.copy(), dS.copy()
                    atw[T - 1] = 0
                    dSw[T - 1] = 0
                out["dk"][rows, cols] = chain3(_split_or_one(T_(dSw), one), q, acc).astype(f)
                out["dv"][rows, cols] = chain3(_split_or_one(T_(atw), mutant == "at_one_plane"), g, acc).astype(f)
            r0 += T
    return out
