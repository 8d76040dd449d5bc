"""CPU: the specification of the streaming attention's training form and backward (tests/attn_stream_bwd_ref.py) pinned to torch.autograd in
float64 under replayed dropout masks, the identity behind delta, the new C entries (declared, bound, exported; their refusals happen before
anything touches a device; their workspace queries are host arithmetic), and the float32 specification finite on every finite family of the
GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import attn_stream_bwd_cases as cases
from attn_stream_bwd_ref import keep_mask, mha_train

NEW = ("sumk_attn_stream_train", "sumk_attn_stream_backward", "sumk_attn_stream_backward_workspace_bytes",
       "sumk_transformer_stream_train_workspace_bytes", "sumk_transformer_forward_stream_train", "sumk_transformer_backward_stream")


def _off(lens):
    return (C.c_int32 * (len(lens) + 1))(0, *np.cumsum(lens).tolist())


@pytest.fixture(scope="module")
def lib():
    from summarizer_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_float64_spec_matches_torch_autograd(p):
    lens, D, heads, seed, site = (1, 64, 65, 33), 24, 2, 99, 13
    rng = np.random.default_rng(5)
    q, k, v, g = (rng.standard_normal((sum(lens), D)) for _ in range(4))
    dh = D // heads
    sc = 1.0 / np.sqrt(dh)
    got = mha_train(q, k, v, g, lens, heads, sc, p, seed, site)
    r0 = 0
    for T in lens:
        t = [torch.from_numpy(a[r0:r0 + T].copy()).requires_grad_(True) for a in (q, k, v)]
        ctx = []
        for h in range(heads):
            cols = slice(h * dh, (h + 1) * dh)
            a = torch.softmax(t[0][:, cols] @ t[1][:, cols].T * sc, dim=1)
            keep = torch.from_numpy(keep_mask(seed, site, p, r0, T, heads, h))
            if p > 0:
                assert 0 < int(keep.sum()) < keep.numel() or T == 1
            a = torch.where(keep, a / (1 - float(np.float32(p))), torch.zeros((), dtype=torch.float64))
            ctx.append(a @ t[2][:, cols])
        ctx = torch.cat(ctx, dim=1)
        (ctx * torch.from_numpy(g[r0:r0 + T])).sum().backward()
        rows = slice(r0, r0 + T)
        assert np.abs(got["ctx"][rows] - ctx.detach().numpy()).max() <= 1e-12
        for name, ten in (("dq", t[0]), ("dk", t[1]), ("dv", t[2])):
            assert np.abs(got[name][rows] - ten.grad.numpy()).max() <= 1e-12, (name, T)
        r0 += T


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_delta_identity_holds_under_dropout(p):
    """delta_i = dctx_i . ctx_i = sum_j dA_ij alpha_ij with dA the masked, rescaled dctx V^T: the row kernel may take the first form."""
    c = cases.with_grad(cases.fwd.case("delta", (70, 130), 64, 2, 11), p)
    out = mha_train(c["q"], c["k"], c["v"], c["dctx"], c["lens"], 2, cases.fwd.scale_of(c), p, cases.SEED, cases.SITE)
    assert np.abs(out["delta"] - out["delta_alt"]).max() <= 1e-12 * max(1.0, np.abs(out["delta"]).max())


def test_new_symbols_are_declared_bound_and_exported(lib):
    from conftest import ROOT
    from summarizer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sumk.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib._SIGS, name
        assert getattr(lib, name) is not None, name
    for tag in ("PROF_ATTN_STREAM_TRAIN", "PROF_ATTN_STREAM_BWD_DELTA", "PROF_ATTN_STREAM_BWD_DQ", "PROF_ATTN_STREAM_BWD_DKV"):
        m = re.search(r"#define SUMK_%s (\d+)" % tag, hdr)
        assert m and int(m.group(1)) == getattr(_lib, tag) < _lib.PROF_NTAGS, tag


def _bwd(lib, D=64, heads=2, lens=(10,), ld=None, p=0.0, ptr=0x10000, dq=None, nb=1 << 20):
    ld = D if ld is None else ld
    return lib.sumk_attn_stream_backward(ptr, ld, ptr, ld, ptr, ld, ptr, ld, ptr, ld, ptr, D, heads, len(lens), _off(list(lens)), ptr, 0.125, p, 1, 0,
                                         ptr if dq is None else dq, ld, ptr, ld, ptr, ld, ptr, nb, None)


def _fwd(lib, D=64, heads=2, lens=(10,), ld=None, p=0.0, ptr=0x10000, q=None, nb=1 << 20):
    ld = D if ld is None else ld
    return lib.sumk_attn_stream_train(ptr if q is None else q, ld, ptr, ld, ptr, ld, D, heads, len(lens), _off(list(lens)), ptr, 0.125, p, 1, 0,
                                      ptr, ld, ptr, ptr, nb, None)


def test_refusals_happen_before_any_device_work(lib):
    """Every call below carries pointers that no device owns: a refusal that came after a launch or a copy would fault, not return."""
    for call in (_bwd, _fwd):
        assert call(lib, D=12) == -1 and b"head width 6" in lib.sumk_last_error()
        assert call(lib, lens=(0,)) == -1 and b"video 0 has 0 frames" in lib.sumk_last_error()
        assert call(lib, lens=(1 << 20,)) == -1 and b"limit 2^20" in lib.sumk_last_error()
        for p in (-0.1, 1.0, 1.5, float("nan")):
            assert call(lib, p=p) == -1 and b"must lie in [0, 1)" in lib.sumk_last_error(), p
        assert call(lib, ld=60) == -1 and b"must be at least D=64" in lib.sumk_last_error()
        assert call(lib, ld=66) == -1 and b"multiple" in lib.sumk_last_error()
        assert call(lib, nb=16) == -2 and b"workspace 16 < required" in lib.sumk_last_error()
    assert _bwd(lib, D=512) == -1 and b"head width 256" in lib.sumk_last_error()
    assert _bwd(lib, dq=0x10004) == -1 and b"16-byte aligned" in lib.sumk_last_error()
    assert _fwd(lib, q=0x10004) == -1 and b"16-byte aligned" in lib.sumk_last_error()
    assert _fwd(lib, D=1040) == -1 and b"head width 520" in lib.sumk_last_error()
    # the transformer entries: exact fp32 only, the head width named
    assert lib.sumk_transformer_stream_train_workspace_bytes(2048, 2048, 8, 2, 1, _off([100])) == 0 and b"head width 256" in lib.sumk_last_error()
    assert lib.sumk_transformer_stream_train_workspace_bytes(1024, 1024, 8, 0, 1, _off([100])) == 0
    assert lib.sumk_attn_stream_backward_workspace_bytes(512, 2, 1, _off([10])) == 0 and b"head width 256" in lib.sumk_last_error()


def test_backward_workspace_is_descriptors_plus_delta(lib):
    assert lib.sumk_attn_stream_backward_workspace_bytes(1024, 8, 1, _off([65536])) == 256 + 65536 * 8 * 4
    assert lib.sumk_attn_stream_backward_workspace_bytes(64, 2, 3, _off([5, 6, 7])) == 256 + 256


def test_stream_training_workspace_never_exceeds_dense(lib):
    seen = set()
    for fam in cases.fwd.families().values():
        for c in fam:
            key = (tuple(c["lens"]), c["D"], c["heads"])
            if key in seen or c["D"] // c["heads"] > 128:
                continue
            seen.add(key)
            for layers in (1, 6):
                off = _off(list(c["lens"]))
                s = lib.sumk_transformer_stream_train_workspace_bytes(c["D"], c["D"], c["heads"], layers, len(c["lens"]), off)
                d = lib.sumk_transformer_workspace_bytes(c["D"], c["D"], c["heads"], layers, len(c["lens"]), off, 1)
                assert 0 < s <= d, (key, layers, s, d)
    assert len(seen) > 100


def test_a_two_hour_video_trains_in_16_gib(lib):
    """One video of 32 768 steps, D = F = 1024, 8 heads, 6 layers.  Dense: alpha and dropout(alpha) alone are 6 x 2 x 8 x 32768^2 x 4 bytes =
    412 GB.  Stream: about 9 row-sized arrays of 1024 floats per layer (q | k | v = 3, ctx, two pre-norm sums, two norm outputs, the
    feed-forward activation) = 7.2 GB over 6 layers, plus the backward's scratch (three gradients, dqkv, dff, ...) of about 1.6 GB."""
    off = _off([32768])
    dense = lib.sumk_transformer_workspace_bytes(1024, 1024, 8, 6, 1, off, 1)
    stream = lib.sumk_transformer_stream_train_workspace_bytes(1024, 1024, 8, 6, 1, off)
    assert dense > 288e9, dense
    assert 0 < stream < 16 * 2 ** 30, stream


def test_float32_spec_is_finite_on_every_finite_family():
    n = 0
    for name, fam in cases.families().items():
        for c in fam:
            s64, s32 = cases.spec(c)
            for k in ("ctx", "dq", "dk", "dv"):
                assert np.isfinite(s32[k]).all() and np.isfinite(s64[k]).all(), (name, c["name"], k)
            n += 1
    assert n == 16 * 10 + len(cases.ragged()) + len(cases.spikes())
