"""The input families of tests/test_gpu_attn_stream.py, built on the host so that tests/test_attn_stream_host.py can check them (workspace
sizes, a finite float32 specification) without a GPU.  TEST INFRASTRUCTURE ONLY.

A case is a dict: name, lens, D, heads, scale (None = 1 / sqrt(dh)), q, k, v (float32 arrays (sum(lens), D)); a spike case also carries
spike_key (the scaled K row) and spike_where (its name among the chosen positions)."""
import math

import numpy as np

STRIP_T = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 320)      # 32-row wave blocks, 64-key tiles, a 128-row strip
STRIP_SHAPES = ((16, 4), (32, 4), (72, 2), (200, 2), (128, 1), (256, 2), (512, 2))    # (D, heads): dh = 4, 8, 36, 100, 128, 128, 256
RAGGED_LENS = ((1, 64, 65, 200, 3, 129), tuple(int(t) for t in np.random.default_rng(90).integers(1, 91, 40)))


def edge_frames(T):
    ks = {0, T - 1}
    ks.update(k for k in (31, 32, 63, 64, 127, 128, 191, 192, 255, 256) if k < T)
    last = (T - 1) // 64 * 64
    ks.update(k for k in (last, last - 1) if 0 <= k < T)
    return sorted(ks)


def _qkv(lens, D, seed, edges=True):
    rng = np.random.default_rng(seed)
    x = [rng.standard_normal((sum(lens), D)).astype(np.float32) for _ in range(3)]
    if edges:                                   # edge frames carry 4x the features: a dropped or doubled key moves a row far past the gate
        r0 = 0
        for T in lens:
            idx = [r0 + k for k in edge_frames(T)]
            for a in x[1:]:
                a[idx] *= 4.0
            r0 += T
    return x


def case(name, lens, D, heads, seed, scale=None, edges=True):
    q, k, v = _qkv(lens, D, seed, edges)
    return dict(name=name, lens=list(lens), D=D, heads=heads, scale=scale, q=q, k=k, v=v)


def scale_of(c):
    return 1.0 / math.sqrt(c["D"] // c["heads"]) if c["scale"] is None else c["scale"]


def strips(D, heads):
    return [case(f"strips_T{T}_D{D}_h{heads}", (T,), D, heads, 1000 + T + D) for T in STRIP_T]


def ragged():
    return [case(f"ragged{i}_D{D}_h8", lens, D, 8, 50 + i) for i, lens in enumerate(RAGGED_LENS) for D in (256, 1024)]


def spikes():
    """Inputs that force the running rescale: one K row scaled so that the row maximum of every query with a positive dot product jumps
    by about J at a chosen key; a staircase (every tile raises the maximum); a spike under which every other weight underflows to 0."""
    out = []
    D, heads = 256, 2                           # dh = 128
    for T in (200, 321):
        # the last tile is partial at both T (keys 192 .. 199; key 320 alone): a key inside it, the very last one when it holds fewer than 3
        keys = {"first": 0, "tile2_first": 64, "mid_tile_last": 127, "last_partial": max((T - 1) // 64 * 64, T - 3)}
        for where, j in keys.items():
            for J in (20, 60, 120):
                c = case(f"spike_T{T}_{where}_J{J}", (T,), D, heads, 7000 + T + j + J, edges=False)
                c["k"][j] *= float(J)          # scale q . k_j ~ N(0, 1) before: J |N(0, 1)| after
                c["spike_key"], c["spike_where"] = j, where
                out.append(c)
        c = case(f"stair_T{T}", (T,), D, heads, 7100 + T, edges=False)
        rng = np.random.default_rng(7200 + T)
        u = rng.standard_normal(D).astype(np.float32)
        u *= np.float32(math.sqrt(3.0 * math.sqrt(128.0)) / np.linalg.norm(u[:128]))      # scale u_h . u_h ~ 3 per head and step
        c["q"] = (0.3 * c["q"] + u).astype(np.float32)
        c["k"] = (0.3 * c["k"] + (1.0 + (np.arange(T) // 64)[:, None]) * u).astype(np.float32)
        out.append(c)
        c = case(f"underflow_T{T}", (T,), D, heads, 7300 + T, edges=False)
        c["spike_key"], c["spike_where"] = 70, "underflow"
        c["k"][70] *= 400.0                     # the other weights are exp(-hundreds) = 0 in float32 for a query with a positive dot
        out.append(c)
    return out


def families():
    fam = {f"strips_D{D}_h{h}": strips(D, h) for D, h in STRIP_SHAPES}
    fam["ragged"] = ragged()
    fam["spike"] = spikes()
    return fam
