"""The dense layer (sumk_linear_forward / _backward), the frame head (sumk_frame_head_forward / _backward) and the shared machinery
only they reach at arbitrary shapes -- the 128x128 buffer-load GEMM with partial tiles, the fp32 split-K weight gradient, the
bias-gradient column sums -- against plain float64 on the CPU (torch, from the fp32 inputs cast up):
  y = x w^T + b      dx = dy w      dw = dw0 + dy^T x      db = db0 + sum_rows dy
  s = sigmoid(h . w + b)      du = ds s (1 - s)      dh = du w      dw = dw0 + sum_rows du h      db = db0 + sum_rows du
The models call these entry points with N, K in {256, 512, 1024} and a handful of row counts, so every branch below is taken one way
only (or never) by the rest of the suite.  The cases are read off the dispatch in csrc/lstm.hip (sumk_linear_*), csrc/gemm_f32.hip
(launch_gemm, gemm_tn_splitk_accum_multi, colsum_multi) and csrc/gemm_regstage.h; the tables next to FWD_CASES and BWD_CASES say what
each row runs.

Gates are element-wise, the ones tests/test_gpu_vasnet.py applies to the plain GEMM, with every added term in the magnitude:
  |got - ref| <= tol x (sum of the absolute values of the terms) + 1e-6,   tol = 2e-6 (fp32, bf16x6), 2^-15 (bf16x3), 2^-7 (bf16);
plain bf16 must also NOT be fp32-exact (is that path really taken?).  That bound grows with K, so at K <= 128 the fp32 forward is also
held to 4 x the error of CPU fp32 torch.nn.functional.linear against the same reference (floor 4 ulps of max |ref|, the form of
test_gpu_optim.py's sumsq gate): on the CPU a sequential fp32 k-chain sits at 0.8-1.0 x that yardstick and an emulated bf16x3 product at
15.6-54 x, so 4 x separates the two.  bf16x6 must stay below 8 x (half the smallest bf16x3 figure).
Every case runs with uninitialised allocations poisoned (0xFF bytes = NaN), so an element nobody wrote fails its gate.

Frame head: the forward gate follows from sigmoid' <= 1/4:  |s - ref| <= 0.25 (2e-6 sum |h||w| + 1e-6) + 2e-7;  dh per element
3e-6 |ref| + 1e-9 max |ref| (fp32 s (1 - s) rounds where float64 does not; four roundings = 2.4e-7 relative);  dw / db
2e-6 (sum_rows |du||h| + |dw0|) + 1e-6.

Measured on MI355X (worst error / gate over all cases; REPORT below, printed per case and written to $SUMK_REPORT_DIR when set):
  forward   fp32 0.26 (4100x1924x100), bf16x6 0.17, bf16x3 0.19 (65x68x32), bf16 0.30 (4100x1924x64);
            fp32 / CPU fp32 yardstick 1.24 x (limit 4; 4100x1796x64 with bias), bf16x6 / yardstick 0.90 x (limit 8; 257x260x100)
  backward  dx 0.18 (fp32, 5000x1024x1024) / 0.23 (bf16), dw 0.10 (fp32, 63x68x36) / 0.11 (bf16x3) / 0.07 (bf16x6) / 0.22 (bf16), db 0.044
  head      scores 0.13 (rows = 1025, F = 4), dh 0.072 (the stated gate needed no widening), dw 0.056, db 0.016
No kernel bug was found; every branch listed below computes what float64 says."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_sumgan_full import Gates, Poison, OUT_GATE, GRAD_GATE

pytestmark = pytest.mark.gpu
F64 = torch.float64
ULP = 2.0 ** -24
TOL = {"fp32": 2e-6, "bf16x6": 2e-6, "bf16x3": 2.0 ** -15, "bf16": 2.0 ** -7}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for r in REPORT:
        print("LINEAR-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "linear_f64.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _randn(shape, seed, scale=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _worst(got, ref, bound):
    """Largest |got - ref| / bound over ALL elements; an element that is NaN (never written) counts as infinitely wrong."""
    got = got.detach().cpu().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(torch.nan_to_num((got - ref).abs() / bound, nan=float("inf")).max())


def _check(gates, what, kind, got, ref, bound, limit=1.0):
    r = _worst(got, ref, bound)
    gates.rows.append((what, kind, r, limit))
    return r


def _finish(gates, **extra):
    worst = {}
    for _, kind, r, limit in gates.rows:
        worst[kind] = max(worst.get(kind, 0.0), r / limit)
    REPORT.append(dict(case=gates.case, worst_over_gate=worst, **extra))
    gates.finish()


# ------------------------------------------------------------------------------------------------ linear forward
# sumk_linear_forward takes 64x64 tiles until gemm_tiles(M, N, 128x128) >= 512, then 128x128 tiles; launch_gemm then picks (fp32):
#   64-tile,  no bias  -> "64 lean":            gemm_lean.hip (plain epilogue, K tail peeled)
#   64-tile,  bias     -> "64 generic + BIAS2": gemm_f32_kernel<64, 64, 32, NT, EPI_BIAS2>
#   128-tile, K % 32 == 0 -> "128 LEAN":        the buffer-load instance, EPI_BIAS2 with a bias / EPI_NONE without
#   128-tile, K % 32 != 0 -> "128 generic":     gemm_f32_kernel<128, 128, 32, NT, EPI_BIAS2 | EPI_NONE>, K tail masked
# and for bf16x3 / bf16x6 / bf16 the "split" instance of the same tile size and epilogue (gemm_split.hip, 2 / 3 / 1 bf16 planes).
FWD_CASES = [
    # (M, N, K)            fp32, no bias | fp32, bias                     what the shape reaches
    (1, 4, 4),           # 64 lean       | 64 generic + BIAS2            smallest legal shape, one k-tile that is all tail
    (5, 8, 36),          # 64 lean       | 64 generic + BIAS2            K tail of 4 behind one whole k-tile
    (65, 68, 32),        # 64 lean       | 64 generic + BIAS2            partial 64-tiles both ways (2 x 2 tiles, 1 row / 4 columns in the last)
    (257, 260, 100),     # 64 lean       | 64 generic + BIAS2            5 x 5 tiles, partial both ways, K % 32 = 4
    (50, 512, 512),      # 64 lean       | 64 generic + BIAS2            SumGAN's mu / logvar shape (1 x 4 tiles of 128 < 512)
    (4100, 1796, 64),    # 64 lean       | 64 generic + BIAS2            33 x 15 = 495 tiles of 128 < 512: still 64-tiles (65 x 29), large
    (4100, 1924, 64),    # 128 LEAN NONE | 128 LEAN + BIAS2              33 x 16 = 528 >= 512; 4100 = 32 x 128 + 4, 1924 = 15 x 128 + 4
    (4100, 1924, 1024),  # 128 LEAN NONE | 128 LEAN + BIAS2              the same tiles over 32 k-tiles
    (4100, 1924, 100),   # 128 generic   | 128 generic + BIAS2           K % 32 != 0: not LEAN, K tail masked
]
FWD_BF16 = {(5, 8, 36), (257, 260, 100), (4100, 1924, 64)}     # plain bf16: one tiny, one 64-tile, one 128-tile case
YARD_MAX_K = 128


def _fwd_inputs(M, N, K):
    seed = 100003 * M + 1009 * N + K
    return _randn((M, K), seed), _randn((N, K), seed + 1), _randn((N,), seed + 2)


@pytest.mark.parametrize("M,N,K", FWD_CASES)
def test_linear_forward_vs_float64(dev, monkeypatch, M, N, K):
    """Every row of FWD_CASES with and without a bias in fp32, bf16x3 and bf16x6 (FWD_BF16: also plain bf16), every element against
    |x||w|^T + |b|; at K <= 128 fp32 and bf16x6 also against the CPU fp32 yardstick (limits 4 x and 8 x).
    Measured on MI355X, error / yardstick per case (1x4x4, 5x8x36, 65x68x32, 257x260x100, 4100x1796x64, 4100x1924x64, 4100x1924x100),
    the larger of bias / no bias: fp32 0.24, 0.62, 0.92, 1.04, 1.24, 0.83, 1.12; bf16x6 0.14, 0.54, 0.62, 0.90, 0.84, 0.75, 0.73."""
    from summarizer_amd import kernels
    x, w, b = _fwd_inputs(M, N, K)
    prod = x.to(F64) @ w.to(F64).T
    mag = x.to(F64).abs() @ w.to(F64).abs().T
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    precisions = ["fp32", "bf16x3", "bf16x6"] + (["bf16"] if (M, N, K) in FWD_BF16 else [])
    gates = Gates(f"linear_forward {M}x{N}x{K}")
    yard_ratio = {}
    for bias in (False, True):
        ref = prod + b.to(F64) if bias else prod
        S = mag + b.to(F64).abs() if bias else mag
        tag = "bias" if bias else "nobias"
        yard = None
        if K <= YARD_MAX_K:
            y32 = F.linear(x, w, b if bias else None)
            yard = max(float((y32.to(F64) - ref).abs().max()), 4 * ULP * float(ref.abs().max()))
        for prec in precisions:
            with Poison(monkeypatch):
                y = kernels.linear_forward(xd, wd, bd if bias else None, prec)
            torch.cuda.synchronize()
            assert y.shape == (M, N)
            _check(gates, f"{prec} {tag}", f"fwd {prec}", y, ref, TOL[prec] * S + 1e-6)
            err = float(torch.nan_to_num((y.cpu().to(F64) - ref).abs(), nan=float("inf")).max())
            if prec == "bf16":
                assert err > 1e-5 * float(ref.abs().max()), "suspiciously exact: is the bf16 path really taken?"
            if yard is not None and prec in ("fp32", "bf16x6"):
                limit = 4.0 if prec == "fp32" else 8.0
                gates.rows.append((f"{prec} {tag} / fp32 yardstick", f"yard {prec}", err / yard, limit))
                yard_ratio[f"{prec} {tag}"] = round(err / yard, 3)
    print(f"\n[linear_forward {M}x{N}x{K}] error / CPU fp32 yardstick: {yard_ratio}")
    _finish(gates, yardstick_ratio=yard_ratio)


@pytest.mark.parametrize("M,N,K", [(96, 160, 72), (4100, 1924, 64)])
def test_linear_forward_exact_integer_data(dev, monkeypatch, M, N, K):
    """Small-integer operands and an integer bias (every product and sum exactly representable, in bf16 too): one case per tile size
    (64-tiles with a K tail; 128-tiles, LEAN in fp32, partial M and N tiles) must be EXACT in all four arithmetics, with and without
    the bias -- a mis-mapped fragment, k pairing, plane or bias column is an exact mismatch."""
    from summarizer_amd import kernels
    A = (np.arange(M * K).reshape(M, K) % 7 - 3).astype(np.float32)
    Bt = ((np.arange(N * K).reshape(N, K) % 5 - 2) + (np.arange(N)[:, None] % 3)).astype(np.float32)
    bias = (np.arange(N) % 11 - 5).astype(np.float32)
    ref = A.astype(np.int64) @ Bt.astype(np.int64).T
    assert np.abs(ref).max() + 5 < 2 ** 24
    xd, wd, bd = torch.from_numpy(A).to(dev), torch.from_numpy(Bt).to(dev), torch.from_numpy(bias).to(dev)
    for prec in ("fp32", "bf16x3", "bf16x6", "bf16"):
        with Poison(monkeypatch):
            y0 = kernels.linear_forward(xd, wd, None, prec)
            y1 = kernels.linear_forward(xd, wd, bd, prec)
        np.testing.assert_array_equal(y0.cpu().numpy(), ref, err_msg=f"{prec} no bias")
        np.testing.assert_array_equal(y1.cpu().numpy(), ref + bias.astype(np.int64)[None, :], err_msg=f"{prec} bias")


@pytest.mark.parametrize("M,N,K", [(257, 260, 100), (4100, 1924, 64)])
def test_linear_forward_writes_nothing_outside_y(dev, M, N, K):
    """Canary: y is a view into a larger NaN buffer with 64 guard rows on each side (through the C ABI, which takes the pointer as it
    is); after the call every guard element is still NaN and the view holds what kernels.linear_forward returns, bit for bit."""
    from summarizer_amd import _lib, kernels
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, w, b = _fwd_inputs(M, N, K)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    G = 64
    ws = torch.full((lib.sumk_linear_workspace_bytes(N, K),), 255, dtype=torch.uint8, device=dev)
    for prec in ("fp32", "bf16x3"):
        for bias in (bd, None):
            want = kernels.linear_forward(xd, wd, bias, prec)
            buf = torch.full((M + 2 * G, N), float("nan"), device=dev)
            y = buf[G:G + M]
            rc = lib.sumk_linear_forward(xd.data_ptr(), wd.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                         M, N, K, ws.data_ptr(), ws.numel(), kernels.precision_code(prec), st)
            _lib.check(rc, "sumk_linear_forward")
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + M:]).all()), (prec, bias is not None, "guard rows written")
            assert torch.equal(y, want), (prec, bias is not None)


# ------------------------------------------------------------------------------------------------ linear backward
# dw: gemm_tn_splitk_accum(dy^T x): an (N, K) product contracted over the M rows.  64-tiles while gemm_tiles(N, K, 128x128) < 64;
# S = min(slots / tiles, ceil(rows / 64), slab 8 N K / (N K) = 8, table 64), kchunk = ceil(rows / S) rounded up to 32, S = ceil(rows /
# kchunk); slab_reduce4_kernel sums the S slabs four at a time plus a tail.  db: colsum_multi: min(128, ceil(rows / 32)) chunks, then
# partial_reduce_multi_kernel (64 partials per pass in 4 loads of 16 groups; 64-column blocks).  dx: the NN GEMM, 64-tiles in every
# row below (fp32: gemm_lean.hip).
BWD_CASES = [
    # (rows, N, K)          tile  S  kchunk  last slice | colsum chunks x rows (last)
    (1, 4, 4),            # 64    1    32       1       |   1 x 1            contraction of length 1 (one video), k-tile tail of 31
    (1, 512, 512),        # 64    1    32       1       |   1 x 1            the same over 8 x 8 tiles; 8 column blocks in the reduce
    (31, 64, 64),         # 64    1    32      31       |   1 x 31           one colsum chunk; contraction one short of a k-tile
    (32, 64, 64),         # 64    1    32      32       |   1 x 32           exactly one k-tile, exactly 32 rows
    (33, 64, 64),         # 64    1    64      33       |   2 x 17 (16)      two chunks; one row into the second k-tile
    (63, 68, 36),         # 64    1    64      63       |   2 x 32 (31)      ceil(rows / 64) = 1
    (64, 68, 36),         # 64    1    64      64       |   2 x 32           ... still 1
    (65, 68, 36),         # 64    2    64       1       |   3 x 22 (21)      ... 2: a last slice of ONE row; ragged 64-column reduce block (68)
    (257, 260, 100),      # 64    5    64       1       |   9 x 29 (25)      ragged everything; slab_reduce4: 4 + tail of 1
    (513, 60, 64),        # 64    6    96      33       |  17 x 31 (17)      17 partials: one full group of 16 + 1; ragged single block (60 columns)
    (2049, 64, 64),       # 64    8   288      33       |  65 x 32 (1)       65 partials: a second 64-partial pass with one partial
    (4096, 128, 32),      # 64    8   512     512       | 128 x 32           the chunk cap, 32 rows each; slab_reduce4: 4 + 4
    (5000, 128, 32),      # 64    8   640     520       | 125 x 40           above the cap: 40 rows per chunk, 125 chunks
    (5000, 896, 1024),    # 64    8   640     520       | 125 x 40           56 tiles of 128 < 64: 64-tile split-K (224 tiles), S capped by the slab
    (5000, 1024, 1024),   # 128   8   640     520       | 125 x 40           64 tiles of 128: 128-tile split-K, S = 8 from the slab
    (700, 1024, 1024),    # 128   8    96      28       |  22 x 32 (28)      kchunk rounding 88 -> 96; last slice shorter than a k-tile
    (400, 1024, 1024),    # 128   7    64      16       |  13 x 31 (28)      S = 7 from ceil(rows / 64): slab_reduce4's 4 + tail of 3 on 128-tiles
]
BWD_ALL_PRECISIONS = {(65, 68, 36), (257, 260, 100), (700, 1024, 1024)}


def _bwd_inputs(M, N, K):
    seed = 200003 * M + 1013 * N + K
    return (_randn((M, K), seed), _randn((N, K), seed + 1), _randn((M, N), seed + 2), _randn((N, K), seed + 3, 3.0),
            _randn((N,), seed + 4, 3.0))


@pytest.mark.parametrize("M,N,K", BWD_CASES)
def test_linear_backward_vs_float64(dev, monkeypatch, M, N, K):
    """Every row of BWD_CASES in fp32 (BWD_ALL_PRECISIONS: also bf16x3, bf16x6, bf16): dx, and dw / db ACCUMULATED onto non-zero
    starting values, every element; a second call from the same starting state gives the same bits."""
    from summarizer_amd import kernels
    x, w, dy, dw0, db0 = _bwd_inputs(M, N, K)
    x64, w64, dy64 = x.to(F64), w.to(F64), dy.to(F64)
    ref_dx, mag_dx = dy64 @ w64, dy64.abs() @ w64.abs()
    ref_dw, mag_dw = dw0.to(F64) + dy64.T @ x64, dy64.abs().T @ x64.abs() + dw0.to(F64).abs()
    ref_db, mag_db = db0.to(F64) + dy64.sum(0), dy64.abs().sum(0) + db0.to(F64).abs()
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
    gates = Gates(f"linear_backward {M}x{N}x{K}")
    for prec in (["fp32", "bf16x3", "bf16x6", "bf16"] if (M, N, K) in BWD_ALL_PRECISIONS else ["fp32"]):
        runs = []
        for _ in range(2):
            dw, db = dw0.clone().to(dev), db0.clone().to(dev)
            with Poison(monkeypatch):
                dx = kernels.linear_backward(xd, wd, dyd, dw, db, True, prec)
            torch.cuda.synchronize()
            runs.append((dx, dw, db))
        (dx, dw, db), (dx2, dw2, db2) = runs
        assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2), (prec, "two identical calls differ")
        _check(gates, f"dx {prec}", f"dx {prec}", dx, ref_dx, TOL[prec] * mag_dx + 1e-6)
        _check(gates, f"dw {prec}", f"dw {prec}", dw, ref_dw, TOL[prec] * mag_dw + 1e-6)
        # the column sums are plain fp32 adds in every arithmetic
        _check(gates, f"db {prec}", "db", db, ref_db, TOL["fp32"] * mag_db + 1e-6)
        if prec == "bf16":
            err = float((dw.cpu().to(F64) - ref_dw).abs().max())
            assert err > 1e-5 * float(ref_dw.abs().max()), "suspiciously exact: is the bf16 path really taken?"
    _finish(gates)


@pytest.mark.parametrize("M,N,K", [(65, 68, 36), (257, 260, 100)])
def test_linear_backward_optional_outputs(dev, monkeypatch, M, N, K):
    """want_dx=False returns None and still accumulates dw and db; db=None (a layer without a bias) leaves dw and dx as they are with
    one: the same bits as the full call, from the same starting state."""
    from summarizer_amd import kernels
    x, w, dy, dw0, db0 = _bwd_inputs(M, N, K)
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
    with Poison(monkeypatch):
        dw_a, db_a = dw0.clone().to(dev), db0.clone().to(dev)
        dx_a = kernels.linear_backward(xd, wd, dyd, dw_a, db_a, True)
        dw_b, db_b = dw0.clone().to(dev), db0.clone().to(dev)
        assert kernels.linear_backward(xd, wd, dyd, dw_b, db_b, False) is None
        dw_c = dw0.clone().to(dev)
        dx_c = kernels.linear_backward(xd, wd, dyd, dw_c, None, True)
    torch.cuda.synchronize()
    assert not torch.equal(dw_a, dw0.to(dev)) and not torch.equal(db_a, db0.to(dev))
    assert torch.equal(dw_b, dw_a) and torch.equal(db_b, db_a)
    assert torch.equal(dw_c, dw_a) and torch.equal(dx_c, dx_a)


# ------------------------------------------------------------------------------------------------ frame head
# forward: four rows per block, one wave per row, a 64-lane float4 loop over F (F = 4: one lane; 252 / 256 / 260: around one full pass;
# 2052: nine passes, the last with one lane).  backward: min(ceil(rows / 4), 256) blocks = up to 1024 waves, above 1024 rows a wave
# owns several; per-wave partials reduced by partial_reduce_kernel (16 groups over the partials, 16 columns per block).
HEAD_F = [4, 252, 256, 260, 512, 2052]
HEAD_ROWS = [1, 3, 4, 5, 1023, 1024, 1025, 5000]


def _head_case(dev, monkeypatch, n_rows, F_, wscale, tag):
    from summarizer_amd import kernels
    seed = 300007 * n_rows + F_
    h = _randn((n_rows, F_), seed)
    w = _randn((1, F_), seed + 1, wscale / np.sqrt(F_))
    b = _randn((1,), seed + 2)
    ds = _randn((n_rows,), seed + 3)
    dw0, db0 = _randn((1, F_), seed + 4, 3.0), _randn((1,), seed + 5, 3.0)
    h64, w64 = h.to(F64), w.to(F64)
    ref_s = torch.sigmoid(h64 @ w64[0] + b.to(F64))
    mag_s = h64.abs() @ w64[0].abs()
    hd, wd, bd, dsd = h.to(dev), w.to(dev), b.to(dev), ds.to(dev)
    gates = Gates(f"frame_head{tag} rows={n_rows} F={F_}")
    with Poison(monkeypatch):
        s = kernels.frame_head_forward(hd, wd, bd)
        s2 = kernels.frame_head_forward(hd, wd, bd)
    assert s.shape == (n_rows,) and torch.equal(s, s2)
    _check(gates, "scores", "scores", s, ref_s, 0.25 * (2e-6 * mag_s + 1e-6) + 2e-7)
    # backward from the scores the forward call returned (what FrameHeadFunction saves), the reference from the same values cast up
    s64 = s.cpu().to(F64)
    du = ds.to(F64) * s64 * (1 - s64)
    ref_dh = du[:, None] * w64
    ref_dw = dw0.to(F64) + (du[:, None] * h64).sum(0, keepdim=True)
    ref_db = db0.to(F64) + du.sum().reshape(1)
    mag_dw = (du.abs()[:, None] * h64.abs()).sum(0, keepdim=True) + dw0.to(F64).abs()
    mag_db = du.abs().sum().reshape(1) + db0.to(F64).abs()
    runs = []
    for _ in range(2):
        dw, db = dw0.clone().to(dev), db0.clone().to(dev)
        with Poison(monkeypatch):
            dh = kernels.frame_head_backward(hd, s, dsd, wd, dw, db)
        torch.cuda.synchronize()
        runs.append((dh, dw, db))
    (dh, dw, db), (dh2, dw2, db2) = runs
    assert torch.equal(dh, dh2) and torch.equal(dw, dw2) and torch.equal(db, db2), "two identical calls differ"
    top = float(ref_dh.abs().max())
    assert top > 0, "reference dh is zero"
    _check(gates, "dh", "dh", dh, ref_dh, 3e-6 * ref_dh.abs() + 1e-9 * top)
    _check(gates, "dw", "dw", dw, ref_dw, 2e-6 * mag_dw + 1e-6)
    _check(gates, "db", "db", db, ref_db, 2e-6 * mag_db + 1e-6)
    _finish(gates)
    return s


@pytest.mark.parametrize("n_rows", HEAD_ROWS)
@pytest.mark.parametrize("F_", HEAD_F)
def test_frame_head_vs_float64(dev, monkeypatch, n_rows, F_):
    """h ~ N(0, 1), w ~ N(0, 1 / sqrt(F)), random b and dscores, non-zero starting dw / db; poisoned workspace; two runs bit-equal.
    Worst error / gate measured on MI355X over the 48 cases: scores 0.13, dh 0.072, dw 0.056, db 0.016."""
    _head_case(dev, monkeypatch, n_rows, F_, 1.0, "")


def test_frame_head_saturated_scores(dev, monkeypatch):
    """w scaled x 40: the logits have a spread of 40, so scores reach exactly 0 and 1 in fp32 (and du = 0 there); same gates."""
    s = _head_case(dev, monkeypatch, 1025, 260, 40.0, " saturated")
    assert bool((s == 0).any()) and bool((s == 1).any()), "the case is meant to saturate on both sides"


# ------------------------------------------------------------------------------------------------ autograd wrappers
def _two_passes(build, leaves, cws):
    """loss_i = sum(build() * cw_i) for two cotangents, backward twice WITHOUT zeroing in between: returns (output, grads of the leaves)."""
    out = None
    for cw in cws:
        out = build()
        (out * cw.to(out.device, out.dtype)).sum().backward()
    return out.detach(), [p.grad for p in leaves]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_linear_function_vs_float64_autograd(dev, monkeypatch, bias):
    """LinearFunction on a 3-D input (T, B, K) against F.linear in float64 on the same graph; the second backward pass finds .grad
    populated (the wrapper then accumulates in place): .grad must hold the SUM of both passes."""
    from summarizer_amd.autograd import LinearFunction
    T, B, K, N = 7, 5, 36, 68
    x, w, b = _randn((T, B, K), 41), _randn((N, K), 42, 0.3), _randn((N,), 43)
    cws = [_randn((T, B, N), 44), _randn((T, B, N), 45)]
    r = [t.to(F64).requires_grad_(True) for t in ((x, w, b) if bias else (x, w))]
    ref_y, ref_g = _two_passes(lambda: F.linear(r[0], r[1], r[2] if bias else None), r, cws)
    g = [t.to(dev).requires_grad_(True) for t in ((x, w, b) if bias else (x, w))]
    with Poison(monkeypatch):
        y, got_g = _two_passes(lambda: LinearFunction.apply(g[0], g[1], g[2] if bias else None, "fp32"), g, cws)
    gates = Gates(f"LinearFunction bias={bias}")
    assert y.shape == (T, B, N)
    gates.fwd("y", y, ref_y, OUT_GATE)
    for name, got, ref in zip(("x", "w", "b"), got_g, ref_g):
        assert got is not None and got.shape == ref.shape, name
        gates.grad(f"d{name}", got, ref, GRAD_GATE["fp32"])
    gates.finish()


def test_frame_head_function_vs_float64_autograd(dev, monkeypatch):
    """FrameHeadFunction against sigmoid(F.linear(h, w, b))[:, 0] in float64, two backward passes without zeroing."""
    from summarizer_amd.autograd import FrameHeadFunction
    n, F_ = 37, 260
    h, w, b = _randn((n, F_), 51), _randn((1, F_), 52, 1 / np.sqrt(F_)), _randn((1,), 53)
    cws = [_randn((n,), 54), _randn((n,), 55)]
    r = [t.to(F64).requires_grad_(True) for t in (h, w, b)]
    ref_s, ref_g = _two_passes(lambda: torch.sigmoid(F.linear(r[0], r[1], r[2]))[:, 0], r, cws)
    g = [t.to(dev).requires_grad_(True) for t in (h, w, b)]
    with Poison(monkeypatch):
        s, got_g = _two_passes(lambda: FrameHeadFunction.apply(g[0], g[1], g[2]), g, cws)
    gates = Gates("FrameHeadFunction")
    assert s.shape == (n,)
    gates.fwd("scores", s, ref_s, OUT_GATE)
    for name, got, ref in zip(("h", "w", "b"), got_g, ref_g):
        assert got is not None and got.shape == ref.shape, name
        gates.grad(f"d{name}", got, ref, GRAD_GATE["fp32"])
    gates.finish()
