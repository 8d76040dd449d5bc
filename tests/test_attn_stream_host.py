"""CPU: the specification of the streaming multi-head attention (tests/attn_stream_ref.py) pinned to the oracle and to torch in float64, the
spike inputs of the GPU tests checked on the float32 specification itself, and the workspace queries of the stream path (host arithmetic:
no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_stream_cases as cases
from attn_stream_ref import mha


def _off(lens):
    return (C.c_int32 * (len(lens) + 1))(0, *np.cumsum(lens).tolist())


@pytest.fixture(scope="module")
def lib():
    from summarizer_amd import _lib
    return _lib.load()


def test_float64_spec_matches_the_oracle_mha():
    """oracle/transformer_np._mha with random in-projection weights and an identity out-projection is the attention of the q, k, v it forms."""
    from oracle import transformer_np
    rng = np.random.default_rng(3)
    T, D, heads = 77, 48, 4
    x = rng.standard_normal((T, D))
    p = {"self_attn.in_proj_weight": rng.standard_normal((3 * D, D)) * 0.3, "self_attn.in_proj_bias": rng.standard_normal(3 * D) * 0.1,
         "self_attn.out_proj.weight": np.eye(D), "self_attn.out_proj.bias": np.zeros(D)}
    want = transformer_np._mha(x, p, "", heads, np.float64)
    qkv = x @ p["self_attn.in_proj_weight"].T + p["self_attn.in_proj_bias"]
    ctx, _ = mha(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], [T], heads, 1.0 / np.sqrt(D // heads))
    assert np.abs(ctx - want).max() <= 1e-12


@pytest.mark.parametrize("lens,D,heads", [((1, 64, 65, 200, 3, 129), 64, 4), ((33,), 72, 2)])
def test_float64_spec_matches_torch_sdpa(lens, D, heads):
    rng = np.random.default_rng(5)
    q, k, v = (rng.standard_normal((sum(lens), D)) for _ in range(3))
    dh = D // heads
    ctx, lse = mha(q, k, v, lens, heads, 1.0 / np.sqrt(dh))
    r0 = 0
    for T in lens:
        t = [torch.from_numpy(a[r0:r0 + T]).view(T, heads, dh).transpose(0, 1) for a in (q, k, v)]
        want = torch.nn.functional.scaled_dot_product_attention(*t).transpose(0, 1).reshape(T, D).numpy()
        assert np.abs(ctx[r0:r0 + T] - want).max() <= 1e-12
        ref_lse = torch.logsumexp(t[0] @ t[1].transpose(1, 2) / np.sqrt(dh), dim=2).t().numpy()
        assert np.abs(lse[r0:r0 + T] - ref_lse).max() <= 1e-12
        r0 += T


def test_spec_nan_rules():
    """NaN in a Q row: that row, every head.  NaN in a K row: every row of the video, the head whose columns hold it.  Other videos: untouched."""
    c = cases.case("nan", (70, 130, 40), 64, 2, 11)
    base, _ = mha(c["q"], c["k"], c["v"], c["lens"], 2, cases.scale_of(c))
    q = c["q"].copy(); q[100] = np.nan
    got, _ = mha(q, c["k"], c["v"], c["lens"], 2, cases.scale_of(c))
    assert np.isnan(got[100]).all() and np.array_equal(np.delete(got, 100, 0), np.delete(base, 100, 0))
    k = c["k"].copy(); k[150, 40] = np.nan
    got, _ = mha(c["q"], k, c["v"], c["lens"], 2, cases.scale_of(c))
    assert np.isnan(got[70:200, 32:]).all() and not np.isnan(got[70:200, :32]).any()
    assert np.array_equal(got[:70], base[:70]) and np.array_equal(got[200:], base[200:])


def test_spike_inputs_keep_the_float32_spec_finite():
    """The spike family must test the kernel, not break the yardstick: the float32 specification stays finite on it and within 1e-4 of the
    float64 one relative to the largest value; the spikes do raise the row maximum late in the walk."""
    for c in cases.spikes():
        sc = cases.scale_of(c)
        c64, l64 = mha(c["q"], c["k"], c["v"], c["lens"], c["heads"], sc)
        c32, l32 = mha(c["q"], c["k"], c["v"], c["lens"], c["heads"], sc, np.float32)
        assert np.isfinite(c32).all() and np.isfinite(l32).all() and np.isfinite(c64).all(), c["name"]
        assert np.abs(c32 - c64).max() <= 1e-4 * np.abs(c64).max(), c["name"]
        assert np.abs(l32 - l64).max() <= 1e-4 * np.abs(l64).max(), c["name"]
        if c.get("spike_key", 0) > 0:                          # every spike but the one at key 0
            s = (c["q"][:, :128].astype(np.float64) @ c["k"][:, :128].astype(np.float64).T) * sc
            late = s.argmax(axis=1) == c["spike_key"]           # rows whose maximum arrives at the spike, after the first tile
            assert c["spike_key"] >= 64 and late.mean() > 0.3, (c["name"], late.mean())
        if c.get("spike_where") == "last_partial":             # a key of the LAST, partial tile (T = 321: key 320, alone in its tile)
            T = c["lens"][0]
            assert T % 64 != 0 and (T - 1) // 64 * 64 <= c["spike_key"] < T, (c["name"], c["spike_key"])
        if c.get("spike_where") == "tile2_first":
            assert c["spike_key"] == 64
        if c.get("spike_where") == "mid_tile_last":
            assert c["spike_key"] % 64 == 63 and c["spike_key"] + 64 < c["lens"][0]
    assert sorted({c["spike_where"] for c in cases.spikes() if "spike_where" in c}) == ["first", "last_partial", "mid_tile_last", "tile2_first", "underflow"]
    assert [c["spike_key"] for c in cases.spikes() if c["name"] == "spike_T321_last_partial_J120"] == [320]
    c = [c for c in cases.spikes() if c["name"] == "stair_T321"][0]
    s = (c["q"][:, :128].astype(np.float64) @ c["k"][:, :128].astype(np.float64).T) * cases.scale_of(c)
    tile_max = np.stack([s[:, t:t + 64].max(axis=1) for t in range(0, 321, 64)], axis=1)
    assert (np.diff(tile_max, axis=1) > 0).mean() > 0.9                 # every tile raises the maximum
    c = [c for c in cases.spikes() if c["name"] == "underflow_T200"][0]
    e = (c["q"][:, :128] @ c["k"][:, :128].T) * np.float32(cases.scale_of(c))
    p = np.exp(e - e.max(axis=1, keepdims=True))
    assert ((p > 0).sum(axis=1) == 1).mean() > 0.3                      # rows whose other weights are exactly 0 in float32


def test_workspace_queries_on_the_host(lib):
    off = _off([65536])
    stream = lib.sumk_transformer_stream_workspace_bytes(1024, 1024, 8, 6, 1, off)
    dense = lib.sumk_transformer_workspace_bytes(1024, 1024, 8, 6, 1, off, 0)
    assert 0 < stream < 8 * 2 ** 30, stream
    assert dense > 100e9, dense
    assert lib.sumk_attn_stream_workspace_bytes(1024, 8, 1, off) == 256
    assert lib.sumk_attn_stream_workspace_bytes(1024, 8, 300, _off([5] * 300)) == 300 * 16 + (-300 * 16) % 256
    # refusals: head width 260 and 6, T = 0, T = 2^20, too many videos, no layers
    assert lib.sumk_attn_stream_workspace_bytes(520, 2, 1, _off([10])) == 0 and b"head width 260" in lib.sumk_last_error()
    assert lib.sumk_attn_stream_workspace_bytes(12, 2, 1, _off([10])) == 0 and b"head width 6" in lib.sumk_last_error()
    assert lib.sumk_attn_stream_workspace_bytes(64, 2, 2, _off([10, 0])) == 0 and b"video 1 has 0 frames" in lib.sumk_last_error()
    assert lib.sumk_attn_stream_workspace_bytes(64, 2, 1, _off([1 << 20])) == 0
    assert lib.sumk_attn_stream_workspace_bytes(64, 2, 1, _off([(1 << 20) - 1])) == 256
    assert lib.sumk_attn_stream_workspace_bytes(64, 2, 65536, _off([1] * 65536)) == 0
    assert lib.sumk_transformer_stream_workspace_bytes(1024, 1024, 8, 0, 1, off) == 0
    assert lib.sumk_transformer_stream_workspace_bytes(2080, 2080, 8, 2, 1, _off([10])) == 0          # dh = 260
    assert lib.sumk_transformer_stream_workspace_bytes(2048, 2048, 8, 6, 1, _off([100])) > 0          # dh = 256


def test_stream_workspace_never_exceeds_dense(lib):
    """For every batch of the GPU families (and the model batches of tests/test_gpu_transformer_stream.py)."""
    seen = set()
    batches = [(c["lens"], c["D"], c["heads"]) for fam in cases.families().values() for c in fam]
    batches += [((1, 63, 64, 65, 129, 200, 321), 256, 2), ((300, 150), 1024, 8), ((700,), 256, 2)]
    for lens, D, heads in batches:
        key = (tuple(lens), D, heads)
        if key in seen:
            continue
        seen.add(key)
        for layers in (1, 6):
            off = _off(list(lens))
            s = lib.sumk_transformer_stream_workspace_bytes(D, D, heads, layers, len(lens), off)
            d = lib.sumk_transformer_workspace_bytes(D, D, heads, layers, len(lens), off, 0)
            assert 0 < s <= d, (key, layers, s, d)


def test_profiler_tags_match_the_header():
    """The tag numbers Python callers use (scripts/attn_stream_timing.py through summarizer_amd._lib) are those of include/sumk.h."""
    import os
    import re
    from conftest import ROOT
    from summarizer_amd import _lib
    src = open(os.path.join(ROOT, "include", "sumk.h")).read()
    tags = {k: int(v) for k, v in re.findall(r"#define (SUMK_PROF_[A-Z0-9_]+) (\d+)", src)}
    assert tags["SUMK_PROF_TF_ATTN_DENSE"] == _lib.PROF_TF_ATTN_DENSE and tags["SUMK_PROF_ATTN_STREAM"] == _lib.PROF_ATTN_STREAM
    assert tags["SUMK_PROF_NTAGS"] == _lib.PROF_NTAGS == 1 + max(v for k, v in tags.items() if k != "SUMK_PROF_NTAGS")
    numbers = [v for k, v in tags.items() if k != "SUMK_PROF_NTAGS"]
    assert len(set(numbers)) == len(numbers)
