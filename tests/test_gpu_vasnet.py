"""GPU parity: the HIP VASNet path (through the C ABI) vs the oracle and the committed golden vectors.
Bar (BASELINE.json north_star): per-frame scores within 1e-4 (fp32) of the reference's CPU path."""
import ctypes as C
import numpy as np
import pytest
import torch

import recipes as R
from conftest import load_golden, js

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _model(dev, D, w, **kw):
    from summarizer_amd.models.vasnet import VASNet
    m = VASNet(input_size=D, **kw).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()})
    return m.to(dev)


def _gemm(lib_fn, A, B, M, N, K, dev):
    from summarizer_amd import _lib
    a = torch.from_numpy(A).to(dev); b = torch.from_numpy(B).to(dev)
    c = torch.full((M, N), float("nan"), device=dev)
    _lib.check(lib_fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gemm")
    torch.cuda.synchronize()
    return c.cpu().numpy()


# (2052, 512, 64) and (2176, 1024, 36): tm = 17 tiles of 128 along M with tn = 4 and tn = 8 -- the XCD-aware tile map of the plain entry
# points (launch_gemm: tn % 4 == 0 && tm >= 16), with an odd tm, so the launch walks 72 / 144 virtual tiles for 68 / 136 real ones
XCD_SHAPES = [(2052, 512, 64), (2176, 1024, 36)]


@pytest.mark.parametrize("M,N,K", [(1, 4, 4), (37, 64, 64), (130, 192, 100), (129, 128, 1024), (300, 3072, 1024), (64, 1000, 36), (257, 260, 8)] + XCD_SHAPES)
def test_gemm_layouts_vs_float64(dev, M, N, K):
    from summarizer_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(M * 7 + N)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bt = rng.standard_normal((N, K)).astype(np.float32)      # asymmetric, non-square: catches transposed C writes
    ref = A.astype(np.float64) @ Bt.astype(np.float64).T
    tol = 2e-6 * np.abs(A).astype(np.float64) @ np.abs(Bt).astype(np.float64).T + 1e-6
    got = _gemm(lib.sumk_gemm_nt, A, Bt, M, N, K, dev)
    assert (np.abs(got - ref) <= tol).all(), f"NT max err {np.abs(got-ref).max()}"
    if N % 4 == 0:
        got = _gemm(lib.sumk_gemm_nn, A, np.ascontiguousarray(Bt.T), M, N, K, dev)
        assert (np.abs(got - ref) <= tol).all(), f"NN max err {np.abs(got-ref).max()}"
        if M % 4 == 0:
            got = _gemm(lib.sumk_gemm_tn, np.ascontiguousarray(A.T), np.ascontiguousarray(Bt.T), M, N, K, dev)
            assert (np.abs(got - ref) <= tol).all(), f"TN max err {np.abs(got-ref).max()}"


@pytest.mark.parametrize("M,N,K", [(4, 4, 4), (36, 64, 64), (132, 192, 100), (128, 128, 1024), (300, 3072, 1024), (64, 1000, 36), (260, 260, 8),
                                   (200, 1024, 260)] + XCD_SHAPES)
def test_gemm_bf16x3_vs_float64(dev, M, N, K):
    """Opt-in bf16x3 arithmetic (hi+lo bf16 splits, 3 bf16 MFMAs, fp32 accumulate), all three layouts: each product carries
    ~2^-16 relative error (dropped lo*lo term and the rounding of lo), so the bound is 2^-15 * |A|.|B|^T -- far tighter
    than plain bf16 (2^-8) -- and data that bf16 represents exactly must come out exact (fragment / plane mapping)."""
    from summarizer_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(M * 7 + N)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bt = rng.standard_normal((N, K)).astype(np.float32)
    Ai = (np.arange(M * K).reshape(M, K) % 7 - 3).astype(np.float32)
    Bi = ((np.arange(N * K).reshape(N, K) % 5 - 2) + (np.arange(N)[:, None] % 3)).astype(np.float32)
    for a_np, b_np, exact in ((A, Bt, False), (Ai, Bi, True)):
        ref = a_np.astype(np.float64) @ b_np.astype(np.float64).T
        bound = 2.0 ** -15 * (np.abs(a_np).astype(np.float64) @ np.abs(b_np).astype(np.float64).T) + 1e-6
        for layout, name in ((0, "NT"), (1, "NN"), (2, "TN")):
            a_host = a_np if layout < 2 else np.ascontiguousarray(a_np.T)
            b_host = b_np if layout == 0 else np.ascontiguousarray(b_np.T)
            a = torch.from_numpy(a_host).to(dev); b = torch.from_numpy(b_host).to(dev)
            c = torch.full((M, N), float("nan"), device=dev)
            _lib.check(lib.sumk_gemm_prec(layout, a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, 1, st), "gemm")
            torch.cuda.synchronize()
            got = c.cpu().numpy()
            if exact:
                np.testing.assert_array_equal(got, ref, err_msg=name)
            else:
                assert (np.abs(got - ref) <= bound).all(), f"{name} bf16x3 max err {np.abs(got - ref).max()}"


@pytest.mark.parametrize("M,N,K", [(4, 4, 4), (36, 64, 64), (132, 192, 100), (128, 128, 1024), (300, 3072, 1024), (64, 1000, 36), (200, 1024, 260)] + XCD_SHAPES)
def test_gemm_bf16x6_is_fp32_grade(dev, M, N, K):
    """bf16x6 (three bf16 planes = fp32's 24 significand bits, six bf16 MFMAs per product) must satisfy the SAME bound as the
    exact fp32 MFMA path in test_gemm_layouts_vs_float64, in all three layouts."""
    from summarizer_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(M * 7 + N)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bt = rng.standard_normal((N, K)).astype(np.float32)
    ref = A.astype(np.float64) @ Bt.astype(np.float64).T
    tol = 2e-6 * np.abs(A).astype(np.float64) @ np.abs(Bt).astype(np.float64).T + 1e-6
    worst = {}
    for prec in (0, 2):
        for layout, name in ((0, "NT"), (1, "NN"), (2, "TN")):
            a_host = A if layout < 2 else np.ascontiguousarray(A.T)
            b_host = Bt if layout == 0 else np.ascontiguousarray(Bt.T)
            a = torch.from_numpy(a_host).to(dev); b = torch.from_numpy(b_host).to(dev)
            c = torch.full((M, N), float("nan"), device=dev)
            _lib.check(lib.sumk_gemm_prec(layout, a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, prec, st), "gemm")
            torch.cuda.synchronize()
            err = np.abs(c.cpu().numpy() - ref)
            assert (err <= tol).all(), f"{name} precision {prec} max err {err.max()}"
            worst[(prec, name)] = float((err / tol).max())
    print("worst err / tol:", worst)


def test_gemm_exact_integer_data_asymmetric(dev):
    # exact small-integer operands: any mis-mapped fragment / k pairing shows up as an exact mismatch
    from summarizer_amd import _lib
    lib = _lib.load()
    M, N, K = 96, 160, 72
    A = (np.arange(M * K).reshape(M, K) % 7 - 3).astype(np.float32)
    Bt = ((np.arange(N * K).reshape(N, K) % 5 - 2) + (np.arange(N)[:, None] % 3)).astype(np.float32)
    ref = A.astype(np.int64) @ Bt.astype(np.int64).T
    np.testing.assert_array_equal(_gemm(lib.sumk_gemm_nt, A, Bt, M, N, K, dev), ref)
    np.testing.assert_array_equal(_gemm(lib.sumk_gemm_nn, A, np.ascontiguousarray(Bt.T), M, N, K, dev), ref)
    np.testing.assert_array_equal(_gemm(lib.sumk_gemm_tn, np.ascontiguousarray(A.T), np.ascontiguousarray(Bt.T), M, N, K, dev), ref)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16x6"])
def test_vasnet_small_goldens_all_variants(dev, precision):
    g = load_golden("vasnet_small")
    meta = js(g["meta"])
    worst = 0.0
    for vname, m in meta.items():
        w = {k.split("/w/")[1]: g[k] for k in g.files if k.startswith(f"{vname}/w/")}
        model = _model(dev, 64, w, precision=precision, **m)
        for c in sorted(k.split("/")[-1] for k in g.files if k.startswith(f"{vname}/x/")):
            x = torch.from_numpy(g[f"{vname}/x/{c}"].copy()).to(dev)
            with torch.no_grad():
                y = model(x).cpu().numpy()
            ref = g[f"{vname}/y/{c}"]
            assert y.shape == ref.shape
            np.testing.assert_allclose(y, ref, atol=TOL, rtol=0, equal_nan=True, err_msg=f"{vname} {c}")
            worst = max(worst, float(np.nanmax(np.abs(y - ref))) if np.isfinite(ref).any() else 0.0)
    print("worst |d| over small goldens:", worst)


def test_vasnet_pos_embed_mutates_callers_tensor_like_reference(dev):
    g = load_golden("vasnet_small")
    w = {k.split("/w/")[1]: g[k] for k in g.files if k.startswith("pos_simple/w/")}
    model = _model(dev, 64, w, max_length=64, pos_embed="simple")
    x0 = g["pos_simple/x/T37B1"]
    x = torch.from_numpy(x0.copy()).to(dev)
    with torch.no_grad():
        model(x)
    np.testing.assert_allclose(x.cpu().numpy()[:, 0, :], x0[:, 0, :] + w["pos_embed.weight"][:37], atol=1e-6)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16x6"])
def test_vasnet_full_size_goldens(dev, precision):
    g = load_golden("vasnet_full")
    n = len([k for k in g.files if k.endswith("/cfg")])
    for ci in range(n):
        cfg = js(g[f"c{ci}/cfg"])
        w = R.vasnet_weights(cfg["D"], cfg["wseed"]); x = R.features(cfg["T"], cfg["B"], cfg["D"], cfg["xseed"])
        assert R.digest(w) == cfg["wdigest"] and R.digest({"x": x}) == cfg["xdigest"]
        model = _model(dev, cfg["D"], w, precision=precision, **cfg["kw"])
        with torch.no_grad():
            y = model(torch.from_numpy(x).to(dev)).cpu().numpy()
        np.testing.assert_allclose(y, g[f"c{ci}/y"], atol=TOL, rtol=0, err_msg=str(cfg))
        print(precision, cfg["T"], "max |d| vs reference:", float(np.abs(y - g[f"c{ci}/y"]).max()))


def test_vasnet_packed_ragged_batch_vs_oracle(dev):
    from oracle import vasnet_np
    D = 256
    w = R.vasnet_weights(D, 31)
    lens = [1, 2, 63, 64, 65, 129, 200, 7]
    xs = [R.features(T, 1, D, 40 + i) - 0.1 for i, T in enumerate(lens)]
    for kw, okw in [(dict(), dict()), (dict(attention_aperture=9, ignore_self=True), dict(aperture=9, ignore_self=True))]:
        model = _model(dev, D, w, **kw)
        xp = torch.from_numpy(np.concatenate([x[:, 0, :] for x in xs])).to(dev)
        with torch.no_grad():
            s = model.score_packed(xp, lens).cpu().numpy()
        off = np.concatenate([[0], np.cumsum(lens)])
        for i, x in enumerate(xs):
            ref = vasnet_np.vasnet_forward(x, w, **okw)[:, 0, 0]
            np.testing.assert_allclose(s[off[i]:off[i + 1]], ref, atol=TOL, rtol=0, equal_nan=True, err_msg=f"video {i} T={lens[i]} {kw}")


def test_vasnet_batch_properties_full_size(dev):
    """BASELINE-size properties that need no oracle: scoring is per-video independent (permuting / re-batching the
    videos permutes the scores bit-for-bit) and repeatable.  A video scored ALONE runs the small-batch kernels (round 4), whose
    K order differs: it equals its scores inside the batch to fp32 re-association (1e-5; measured 4e-6), is bit-repeatable, and does not depend
    on which other call preceded it."""
    D = 1024
    model = _model(dev, D, R.vasnet_weights(D, 5))
    rng = np.random.default_rng(0)
    lens = [int(np.ceil(v)) for v in rng.uniform(150, 320, 12)]
    xs = [torch.from_numpy(R.features(T, 1, D, 90 + i)[:, 0, :]).to(dev) for i, T in enumerate(lens)]
    with torch.no_grad():
        a = model.score_packed(torch.cat(xs), lens)
        b = model.score_packed(torch.cat(xs), lens)
        perm = [5, 0, 11, 3, 7, 1, 9, 2, 10, 4, 8, 6]
        c = model.score_packed(torch.cat([xs[i] for i in perm]), [lens[i] for i in perm])
        singles = [model(x.unsqueeze(1))[:, 0, 0] for x in xs]
        singles_again = [model(x.unsqueeze(1))[:, 0, 0] for x in reversed(xs)][::-1]
    assert torch.equal(a, b)
    off = np.concatenate([[0], np.cumsum(lens)]); offp = np.concatenate([[0], np.cumsum([lens[i] for i in perm])])
    for j, i in enumerate(perm):
        assert torch.equal(c[offp[j]:offp[j + 1]], a[off[i]:off[i + 1]])
    for i, s in enumerate(singles):
        assert torch.equal(s, singles_again[i])
        assert float((s - a[off[i]:off[i + 1]]).abs().max()) < 1e-5
    assert bool(((a > 0) & (a < 1)).all())


def test_vasnet_long_sequence_D2048_vs_oracle(dev):
    """BASELINE config 5 shape class (long video, D=2048) at an oracle-checkable length: T=1500, plus a local-attention
    variant (numpy float64-free oracle, op for op); T = 10 000 against the torch port is test_vasnet_full_stress_size_vs_torch_port."""
    from oracle import vasnet_np
    D, T = 2048, 1500
    w = R.vasnet_weights(D, 71)
    x = (R.features(T, 1, D, 72) * 0.1).astype(np.float32)       # N(0,1)*0.05-like magnitude (SURVEY 8d, S-stress)
    for kw, okw in [(dict(), dict()), (dict(attention_aperture=64), dict(aperture=64))]:
        model = _model(dev, D, w, **kw)
        with torch.no_grad():
            y = model(torch.from_numpy(x).to(dev)).cpu().numpy()
        ref = vasnet_np.vasnet_forward(x, w, **okw)
        np.testing.assert_allclose(y, ref, atol=TOL, rtol=0, err_msg=str(kw))


_STRESS_REF = {}


@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "bf16x3"])
def test_vasnet_full_stress_size_vs_torch_port(dev, precision):
    """(round 6: parametrised over the arithmetic -- in bf16x6 / bf16x3 a T >= 1536 video runs its (T x T) products on the plane GEMM
    itself, one launch per product, with the masks applied by csrc/gemm_pw.hip's softmax_planes_kernel; logits gate 5e-2 at two planes.)
    BASELINE config 5 at FULL size against the oracle: ONE (T = 10 000, D = 2048) sequence, default attention and
    attention_aperture = 64, HIP vs oracle/torch_port (vasnet.py:92-148 op for op, ~5 s of CPU per variant): every score within
    1e-4 (north_star's gate) -- and, because these scores saturate (2e-4 ... 0.9998, where 1e-4 on a score is 0.5 on its logit), the
    PRE-SIGMOID values too: logit(score) in float64 against the port's k2 output within 5e-3 wherever |logit| <= 8 (an fp32 score
    at 0.9997 resolves its logit to ~3e-4; the full-T attention -- 79 x 79 tiles of Q.K^T with K = 2048, alpha.V with K = 10 000 --
    feeds these values through two LayerNorms, so an error in it shows up here at size)."""
    from oracle import torch_port
    D, T = 2048, 10000
    from summarizer_amd.models.vasnet import VASNet
    torch.manual_seed(1234)
    base = VASNet(input_size=D)
    p = {k: v.detach().clone() for k, v in base.named_parameters()}
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(T, 1, D, generator=g) * 0.05)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    for kw, okw in [(dict(), dict()), (dict(attention_aperture=64), dict(aperture=64))]:
        m = VASNet(input_size=D, **kw)
        m.load_state_dict(base.state_dict())
        m = m.to(dev).eval()
        m.precision = precision
        key = tuple(sorted(okw.items()))
        with torch.no_grad():
            y = m(x.to(dev)).cpu().double().reshape(-1)
            if key not in _STRESS_REF:                     # (the port's 5 s per variant once for the three arithmetics)
                _STRESS_REF[key] = torch_port.vasnet_scores(x, p, return_logits=True, **okw)
            ref, ref_logit = _STRESS_REF[key]
        ref, ref_logit = ref.double().reshape(-1), ref_logit.double().reshape(-1)
        assert float((y - ref).abs().max()) < TOL, (kw, float((y - ref).abs().max()))
        logit = torch.log(y) - torch.log1p(-y)
        sel = ref_logit.abs() <= 8.0
        assert int(sel.sum()) > T // 2, (kw, int(sel.sum()))
        gate = 5e-2 if precision == "bf16x3" else 5e-3
        assert float((logit - ref_logit)[sel].abs().max()) < gate, (kw, precision, float((logit - ref_logit)[sel].abs().max()))


def test_vasnet_full_stress_size_properties(dev):
    """BASELINE config 5 at FULL size (T = 10 000, D = 2048), properties that need no oracle (the oracle comparison at this size is
    the test above, one sequence; here the batch dimension): (1) batching independence -- two
    long videos scored together equal their separate scores bit for bit; (2) locality of the banded attention -- with
    `local = 64` a frame only sees +-64 neighbours, so scoring the first 6 000 frames alone must reproduce the scores of
    the frames further than 64 from the cut; (3) scores are probabilities."""
    D, T = 2048, 10000
    torch.manual_seed(12)
    g = torch.Generator(device=dev); g.manual_seed(3)
    xs = [torch.randn(T, D, device=dev, generator=g) * 0.05 for _ in range(2)]
    from summarizer_amd.models.vasnet import VASNet
    m = VASNet(input_size=D).to(dev).eval()
    with torch.no_grad():
        both = m.score_packed(torch.cat(xs), [T, T])
        a = m.score_packed(xs[0], [T]); b = m.score_packed(xs[1], [T])
    assert torch.equal(both[:T], a) and torch.equal(both[T:], b)
    assert bool(((both > 0) & (both < 1)).all())
    del both, a, b
    ml = VASNet(input_size=D, attention_aperture=64).to(dev).eval()
    ml.load_state_dict(m.state_dict())
    with torch.no_grad():
        full = ml.score_packed(xs[0], [T])
        head = ml.score_packed(xs[0][:6000].contiguous(), [6000])
    np.testing.assert_allclose(head[:6000 - 65].cpu().numpy(), full[:6000 - 65].cpu().numpy(), atol=2e-6, rtol=0)
    assert float((head[6000 - 64:] - full[6000 - 64:6000]).abs().max()) > 0          # the cut does matter inside the band


@pytest.mark.parametrize("M,N,K", [(4, 4, 4), (132, 192, 100), (300, 3072, 1024), (200, 1024, 260)])
def test_gemm_plain_bf16_vs_float64(dev, M, N, K):
    """precision "bf16" (SUMK_PRECISION_BF16: one bf16 plane, ONE MFMA per product, fp32 accumulate -- the mixed-precision
    training arithmetic): each operand is rounded to 8 significant bits, so a product carries <= 2^-8 + 2^-8 relative error:
    bound 2^-7 * |A|.|B|^T; bf16-representable data must come out exact (fragment / plane mapping) in all three layouts."""
    from summarizer_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(M * 7 + N)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bt = rng.standard_normal((N, K)).astype(np.float32)
    Ai = (np.arange(M * K).reshape(M, K) % 7 - 3).astype(np.float32)
    Bi = ((np.arange(N * K).reshape(N, K) % 5 - 2) + (np.arange(N)[:, None] % 3)).astype(np.float32)
    for a_np, b_np, exact in ((A, Bt, False), (Ai, Bi, True)):
        ref = a_np.astype(np.float64) @ b_np.astype(np.float64).T
        bound = 2.0 ** -7 * (np.abs(a_np).astype(np.float64) @ np.abs(b_np).astype(np.float64).T) + 1e-6
        for layout, name in ((0, "NT"), (1, "NN"), (2, "TN")):
            a_host = a_np if layout < 2 else np.ascontiguousarray(a_np.T)
            b_host = b_np if layout == 0 else np.ascontiguousarray(b_np.T)
            a = torch.from_numpy(a_host).to(dev); b = torch.from_numpy(b_host).to(dev)
            c = torch.full((M, N), float("nan"), device=dev)
            _lib.check(lib.sumk_gemm_prec(layout, a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, 3, st), "gemm")
            torch.cuda.synchronize()
            got = c.cpu().numpy()
            if exact:
                np.testing.assert_array_equal(got, ref, err_msg=name)
            else:
                err = np.abs(got - ref)
                assert (err <= bound).all(), f"{name} bf16 max err {err.max()}"
                assert err.max() > 1e-5 * np.abs(ref).max(), "suspiciously exact: is the bf16 path really taken?"


@pytest.mark.parametrize("wide", [0, 192, 256])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 136, 192), (1000, 3072, 1024), (1024, 1024, 3011), (264, 1024, 12003)])
def test_gemm_bf16_sources_vs_float64(dev, M, N, K, wide, monkeypatch):
    """csrc/gemm_b16.hip: bf16 operands in HBM, fp32 accumulate.  The operands ARE bf16 here, so the only error left is the fp32
    accumulation order: against float64 of the same bf16 values the bound is K * 2^-24 * |A|.|B|^T (a few 1e-6 relative), and small-integer
    data must come out exact -- in all three layouts, on ragged M / N tiles, K tails of the M/N-contiguous operands (zeroed by the
    buffer descriptor, not by masks) and through the deterministic split-K weight-gradient form (C += A^T B twice = 2x).
    wide = 0: 128x128 tiles; 192 / 256: the (BM x 256) double-buffered tiles, forced here on shapes the launcher would give to the
    small tile (ragged M and N tiles, one-tile problems)."""
    from summarizer_amd import _lib
    lib = _lib.load()
    monkeypatch.setenv("SUMK_B16_WIDE", str(wide))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cpu"); g.manual_seed(M * 7 + N + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    B = torch.randn(N, K, generator=g).to(torch.bfloat16)
    Ai = ((torch.arange(M * K).reshape(M, K) % 7) - 3).to(torch.bfloat16)
    Bi = (((torch.arange(N * K).reshape(N, K) % 5) - 2) + (torch.arange(N)[:, None] % 3)).to(torch.bfloat16)
    ws = torch.zeros(8192 + 24 * M * N * 4, dtype=torch.uint8, device=dev)
    for a16, b16, exact in ((A, B, False), (Ai, Bi, True)):
        a64, b64 = a16.double().numpy(), b16.double().numpy()
        ref = a64 @ b64.T
        bound = (K + 64) * 2.0 ** -24 * (np.abs(a64) @ np.abs(b64).T) + 1e-30
        for layout, name in ((0, "NT"), (1, "NN"), (2, "TN")):
            if layout < 2 and K % 64:
                continue                      # a K-contiguous operand needs whole k-tiles (the caller's eligibility check; refused below)
            a = (a16 if layout < 2 else a16.T.contiguous()).to(dev)
            b = (b16 if layout == 0 else b16.T.contiguous()).to(dev)
            c = torch.full((M, N), float("nan"), device=dev)
            _lib.check(lib.sumk_gemm_bf16src(layout, a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, None, 0, st), "gemm_bf16src")
            got = c.cpu().numpy().astype(np.float64)
            if exact:
                np.testing.assert_array_equal(got, ref, err_msg=name)
            else:
                err = np.abs(got - ref)
                assert (err <= bound).all(), f"{name} max err {err.max()} vs bound {bound.flat[err.argmax()]}"
            if layout == 2:                    # split-K, accumulating: two calls on a zeroed C
                c2 = torch.zeros((M, N), device=dev)
                for _ in range(2):
                    _lib.check(lib.sumk_gemm_bf16src(2, a.data_ptr(), b.data_ptr(), c2.data_ptr(), M, N, K, ws.data_ptr(), ws.numel(), st), "gemm_bf16src split-K")
                got2 = c2.cpu().numpy().astype(np.float64)
                if exact:
                    np.testing.assert_array_equal(got2, 2 * ref, err_msg="TN split-K")
                else:
                    assert (np.abs(got2 - 2 * ref) <= 2 * bound + 1e-6 * np.abs(ref)).all(), "TN split-K"
    if K % 64:
        c = torch.zeros((M, N), device=dev)
        with pytest.raises(_lib.SumkError, match="not eligible"):
            _lib.check(lib.sumk_gemm_bf16src(0, A.to(dev).data_ptr(), B.to(dev).data_ptr(), c.data_ptr(), M, N, K, None, 0, st), "gemm_bf16src")


def test_vasnet_plain_bf16_scores_are_close_but_not_fp32_grade(dev):
    """Plain bf16 arithmetic is a TRAINING mode: scores stay within 3e-2 of the reference goldens but miss the 1e-4 scoring gate
    the fp32-grade paths hold -- it is never the default."""
    g = load_golden("vasnet_full")
    worst = 0.0
    for ci in (0, 1, 2):
        cfg = js(g[f"c{ci}/cfg"])
        w = R.vasnet_weights(cfg["D"], cfg["wseed"]); x = R.features(cfg["T"], cfg["B"], cfg["D"], cfg["xseed"])
        model = _model(dev, cfg["D"], w, precision="bf16", **cfg["kw"])
        with torch.no_grad():
            y = model(torch.from_numpy(x).to(dev)).cpu().numpy()
        worst = max(worst, float(np.abs(y - g[f"c{ci}/y"]).max()))
    print("plain bf16: max |d score| vs reference goldens:", worst)
    assert 1e-4 < worst < 3e-2, worst


@pytest.mark.parametrize("precision", ["fp32", "bf16x6"])
def test_vasnet_folded_vo_inference_matches_reference_goldens(dev, precision):
    """fold_vo=True (opt-in): Wvo = Wo.Wv is folded once and the out-projection GEMM disappears.  Same gate as the default
    path: every golden from the REAL reference within 1e-4 -- small-D variants (masks, batch > 1, pos-embed), the full-size
    cases -- and the ragged packed batch within 1e-5 of the unfolded HIP path.  Also in the fp32-grade bf16x6 arithmetic: that
    combination is the fastest mode that still holds the fp32 tolerances (0.74 ms per S-TVSum batch)."""
    g = load_golden("vasnet_small")
    for vname, kw in js(g["meta"]).items():
        w = {k.split("/w/")[1]: g[k] for k in g.files if k.startswith(f"{vname}/w/")}
        m = _model(dev, 64, w, fold_vo=True, **kw)
        m.precision = precision
        if kw.get("pos_embed") == "attention":
            m.pos_embed = torch.from_numpy(g[f"{vname}/pos_table"])
        for c in sorted(k.split("/")[-1] for k in g.files if k.startswith(f"{vname}/x/")):
            with torch.no_grad():
                y = m(torch.from_numpy(g[f"{vname}/x/{c}"].copy()).to(dev)).cpu().numpy()
            np.testing.assert_allclose(y, g[f"{vname}/y/{c}"], atol=TOL, rtol=0, equal_nan=True, err_msg=f"{vname} {c}")
    g = load_golden("vasnet_full")
    for ci in range(len([k for k in g.files if k.endswith("/cfg")])):
        cfg = js(g[f"c{ci}/cfg"])
        w = R.vasnet_weights(cfg["D"], cfg["wseed"]); x = R.features(cfg["T"], cfg["B"], cfg["D"], cfg["xseed"])
        mf = _model(dev, cfg["D"], w, fold_vo=True, **cfg["kw"]); mf.precision = precision
        with torch.no_grad():
            y = mf(torch.from_numpy(x).to(dev)).cpu().numpy()
        np.testing.assert_allclose(y, g[f"c{ci}/y"], atol=TOL, rtol=0, err_msg=str(cfg))
    D, lens = 1024, [70, 1, 33, 129, 300, 5]
    w = R.vasnet_weights(D, 9)
    x = torch.from_numpy(np.concatenate([R.features(T, 1, D, 60 + i)[:, 0, :] - 0.15 for i, T in enumerate(lens)])).to(dev)
    a, b = _model(dev, D, w), _model(dev, D, w, fold_vo=True)
    b.precision = precision
    with torch.no_grad():
        sa, sb_ = a.score_packed(x, lens), b.score_packed(x, lens)
    assert float((sa - sb_).abs().max()) < 1e-5 and not torch.equal(sa, sb_)      # equal up to re-association, and really another path


def test_vasnet_folded_vo_sees_optimiser_steps_without_a_mode_switch(dev):
    """a model that STAYS in eval() (fine-tuning with dropout off; StreamingScorer between steps) while FlatAdam steps it
    through the C ABI -- no train()/eval() switch, no torch-visible version bump -- must not score with a stale Wvo."""
    from summarizer_amd.training import FlatAdam
    D, lens = 128, [40, 17]
    w = R.vasnet_weights(D, 5)
    x = torch.from_numpy(np.concatenate([R.features(T, 1, D, 90 + i)[:, 0, :] for i, T in enumerate(lens)])).to(dev)
    m, ref = _model(dev, D, w, fold_vo=True), _model(dev, D, w)
    opts = [FlatAdam(mm.parameters(), lr=1e-2) for mm in (m, ref)]
    for _ in range(2):
        with torch.no_grad():
            a, b = m.score_packed(x, lens), ref.score_packed(x, lens)        # folded scoring BETWEEN the steps fills the cache
        assert float((a - b).abs().max()) < 1e-5
        for mm, opt in zip((m, ref), opts):                                   # eval mode throughout: gradients still flow
            opt.zero_grad(); (mm.score_packed(x, lens) ** 2).mean().backward(); opt.step()
    with torch.no_grad():
        a, b = m.score_packed(x, lens), ref.score_packed(x, lens)
    assert float((a - b).abs().max()) < 1e-5


def test_vasnet_folded_vo_follows_weight_updates(dev):
    """The folded matrix is a cache of two weights: a training step through the HIP optimiser (invisible to torch's version
    counters), load_state_dict and a plain in-place torch edit must all be picked up by the next scoring call."""
    from summarizer_amd.training import FlatAdam
    D, lens = 128, [40, 17]
    w = R.vasnet_weights(D, 5)
    x = torch.from_numpy(np.concatenate([R.features(T, 1, D, 90 + i)[:, 0, :] for i, T in enumerate(lens)])).to(dev)
    m, ref = _model(dev, D, w, fold_vo=True), _model(dev, D, w)
    def same():
        with torch.no_grad():
            return float((m.score_packed(x, lens) - ref.score_packed(x, lens)).abs().max()) < 1e-5
    assert same()
    for mm in (m, ref):                                        # one identical optimiser step on both models
        mm.train(); mm.dropout.p = 0.0
        opt = FlatAdam(mm.parameters(), lr=1e-2)
        opt.zero_grad(); (mm.score_packed(x, lens) ** 2).mean().backward(); opt.step()
        mm.eval()
    assert same()
    with torch.no_grad():
        for mm in (m, ref):
            mm.V.weight.mul_(1.5)                              # in-place edit in eval mode: caught by the version counter
    assert same()
    sd = {k: torch.from_numpy(v) for k, v in R.vasnet_weights(D, 6).items()}
    m.load_state_dict(sd); ref.load_state_dict(sd)
    assert same()


def test_lean_gemm_equals_generic_kernel(tmp_path):
    """csrc/gemm_lean.hip (the 64x64 per-video products with a VALU-free main loop, persistent tile walk, peeled K tail) against the
    generic register-staged kernel (SUMK_LEAN=0) on a ragged batch -- T = 1 ... 333, inference scores, training-mode scores, dX and
    every parameter gradient -- and on plain NT / NN GEMMs with K tails: BIT-identical (same k order, one fmaf chain per element)."""
    import os, subprocess, sys
    from conftest import ROOT
    probe = os.path.join(ROOT, "scripts", "probes", "lean_equiv.py")
    outs = {}
    for flag in ("1", "0"):
        f = str(tmp_path / f"lean{flag}.npz")
        # (SUMK_SK=0: this batch is small enough for the small-batch path, which has its own test below)
        r = subprocess.run([sys.executable, probe, f], env=dict(os.environ, SUMK_LEAN=flag, SUMK_SK="0"), capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        outs[flag] = np.load(f)
    a, b = outs["1"], outs["0"]
    assert set(a.files) == set(b.files) and len(a.files) > 15
    for k in a.files:
        assert np.isfinite(a[k]).all() or k.startswith("scores"), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_fused_inference_tail_equals_separate_kernels(tmp_path):
    """The fused inference tail (LayerNorm 1 applied to the k1 product, LayerNorm 2 + k2 taken from the k1 epilogue: neither
    activation matrix is stored) against the separate LayerNorm kernels on the S-TVSum batch (50 videos, D = 1024): the
    re-association moves scores by a few 1e-6 at most.  The switches are read once per process, hence the subprocesses."""
    import os, subprocess, sys
    from conftest import ROOT
    probe = os.path.join(ROOT, "scripts", "probes", "fused_tail_diff.py")
    outs = {}
    for tag, env in (("fused", {}), ("head_only", {"SUMK_FUSED_LN": "0"}), ("separate", {"SUMK_FUSED_LN": "0", "SUMK_FUSED_HEAD": "0"})):
        f = str(tmp_path / f"{tag}.npy")
        r = subprocess.run([sys.executable, probe, f], env=dict(os.environ, **env), capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        outs[tag] = np.load(f)
    assert np.isfinite(outs["fused"]).all() and outs["fused"].shape == (12003,)
    assert np.abs(outs["head_only"] - outs["separate"]).max() < 2e-6
    assert np.abs(outs["fused"] - outs["separate"]).max() < 1e-5


def test_small_batch_path_matches_large_batch_kernels(tmp_path):
    """The small-batch path (round 4; taken for batches of <= 1024 frames, i.e. the reference's one-video-per-call pattern,
    vasnet.py:193-212: every GEMM on csrc/gemm_direct.hip -- a 32x32 tile per workgroup, K split over its waves) against the
    large-batch kernels (SUMK_SK=0): ONE T = 300 video at D = 1024, a ragged batch with T = 1 ... 333, three videos with local
    attention + ignore_self, D = 400; eval scores, training-mode scores with dropout, every parameter gradient, with and without dX.  The
    partial sums of a tile's waves are added in wave order, so the two paths agree to fp32 re-association, not bit for bit:
    scores 1e-5 (measured 3e-6 with dropout), gradients 2e-4 of the tensor's largest entry (k2.bias, a cancelling sum over all frames, measured 7e-5; the matrices 1e-6).  The small-batch path itself is bit-repeatable."""
    import os, subprocess, sys
    from conftest import ROOT
    probe = os.path.join(ROOT, "scripts", "probes", "sk_equiv.py")
    outs = {}
    for flag in ("1", "0"):
        f = str(tmp_path / f"sk{flag}.npz")
        r = subprocess.run([sys.executable, probe, f], env=dict(os.environ, SUMK_SK=flag), capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        outs[flag] = np.load(f)
    a, b = outs["1"], outs["0"]
    assert set(a.files) == set(b.files) and len(a.files) > 60
    for tag in ("one", "ragged", "three", "odd"):
        np.testing.assert_array_equal(a[f"{tag}_scores_eval"], a[f"{tag}_scores_eval_again"])
    differs = False
    for k in a.files:
        assert np.isfinite(a[k]).all(), k
        differs = differs or not np.array_equal(a[k], b[k])
        if "scores" in k:
            assert np.abs(a[k] - b[k]).max() < 1e-5, (k, np.abs(a[k] - b[k]).max())
        else:
            assert np.abs(a[k] - b[k]).max() <= 2e-4 * max(np.abs(b[k]).max(), 1e-30), (k, np.abs(a[k] - b[k]).max(), np.abs(b[k]).max())
    assert differs, "bit-identical everywhere: did SUMK_SK select two different paths?"


@pytest.mark.parametrize("M,N,K", [(1, 1, 4), (64, 64, 128), (65, 130, 300), (300, 1024, 1024), (37, 200, 2048), (128, 96, 260), (333, 77, 161)])
def test_gemm_splitk_in_launch_vs_float64(dev, M, N, K):
    """csrc/gemm_lean.hip, SK instances (the small-batch launches of sumk_vasnet_forward / _backward) by themselves through
    sumk_gemm_splitk: NT / NN / TN, 1 ... 8 K slices that meet inside the launch (partial tiles + tickets, last arriver adds in slice
    order), every run-time epilogue, ragged M / N tiles, K tails inside the last slice, more slices asked for than K holds -- against
    float64 with the fp32 dot-product bound, exact on small-integer data, bit-repeatable, and the ticket words left zero (a second
    launch on the same workspace needs no re-initialisation)."""
    from summarizer_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cpu"); g.manual_seed(M * 131 + N * 7 + K)
    Kp, Np, Mp = (K + 3) // 4 * 4, (N + 3) // 4 * 4, (M + 3) // 4 * 4              # leading dimensions in multiples of 4 (16-byte rows)
    a = torch.zeros(M, Kp); a[:, :K] = torch.randn(M, K, generator=g)
    b = torch.zeros(N, Kp); b[:, :K] = torch.randn(N, K, generator=g)
    ai = torch.zeros(M, Kp); ai[:, :K] = ((torch.arange(M * K).reshape(M, K) % 7) - 3).float()
    bi = torch.zeros(N, Kp); bi[:, :K] = (((torch.arange(N * K).reshape(N, K) % 5) - 2) + (torch.arange(N)[:, None] % 3)).float()
    res = torch.randn(M, N, generator=g); bias = torch.randn(N, generator=g)
    for A, B, exact in ((a, b, False), (ai, bi, True)):
        a64, b64 = A[:, :K].double().numpy(), B[:, :K].double().numpy()
        prod = a64 @ b64.T
        bound = (K + 64) * 2.0 ** -23 * (np.abs(a64) @ np.abs(b64).T) + 1e-6
        for layout, name in ((0, "NT"), (1, "NN"), (2, "TN")):
            if layout == 0:
                Ad, Bd, lda, ldb = A.to(dev), B.to(dev), Kp, Kp
            elif layout == 1:
                bt = torch.zeros(K, Np); bt[:, :N] = B[:, :K].t()
                Ad, Bd, lda, ldb = A.to(dev), bt.to(dev), Kp, Np
            else:
                at = torch.zeros(K, Mp); at[:, :M] = A[:, :K].t()
                bt = torch.zeros(K, Np); bt[:, :N] = B[:, :K].t()
                Ad, Bd, lda, ldb = at.to(dev), bt.to(dev), Mp, Np
            for S in (1, 2, 3, 8):
                nb = lib.sumk_gemm_splitk_workspace_bytes(M, N, S)
                ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev).fill_(0xA5)      # poisoned: tickets are initialised by the call
                wsp = (ws.data_ptr() + 255) // 256 * 256
                for epi, ename in ((0, "none"), (1, "residual"), (2, "bias_relu"), (4, "accum")):
                    c0 = torch.randn(M, N, generator=g)
                    Cd = c0.clone().to(dev) if epi == 4 else torch.full((M, N), float("nan"), device=dev)
                    Rd, bd = res.to(dev), bias.to(dev)
                    outs = []
                    for rep in range(2):
                        if epi == 4:
                            Cd.copy_(c0.to(dev))
                        _lib.check(lib.sumk_gemm_splitk(layout, Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr(), M, N, K, lda, ldb, N, S, epi,
                                                        Rd.data_ptr() if epi == 1 else None, N, bd.data_ptr() if epi == 2 else None, 1.0,
                                                        wsp, nb, st), "gemm_splitk")
                        outs.append(Cd.cpu().numpy().astype(np.float64))
                    assert np.array_equal(outs[0], outs[1]), (name, S, ename)
                    want = {0: prod, 1: prod + res.double().numpy(), 2: np.maximum(prod + bias.double().numpy()[None, :], 0.0), 4: c0.double().numpy() + prod}[epi]
                    if exact and epi in (0, 4) and epi == 0:
                        np.testing.assert_array_equal(outs[0], want, err_msg=f"{name} S={S} {ename}")
                    else:
                        assert (np.abs(outs[0] - want) <= bound + 1e-6 * np.abs(want)).all(), (name, S, ename, np.abs(outs[0] - want).max())


def test_prebuilt_problem_tables_equal_per_call_setup(dev):
    """sumk_vasnet_opts.tables (round 4): the batch's problem tables built ONCE per geometry (kernels.vasnet_tables, kept with the SeqBatch)
    against the per-call setup kernels (tables = None): inference and training (scores, every gradient, dX), a single video (small-batch
    path: sliced tables + tickets, used by several consecutive calls) and a 12-video batch (large-batch tables) -- bit-identical, and a
    second SeqBatch of another geometry in between does not disturb the first one's tables."""
    from summarizer_amd import kernels
    from summarizer_amd.autograd import VasnetFunction
    D = 256
    model = _model(dev, D, R.vasnet_weights(D, 9))
    names = [k for _, k in kernels.VASNET_FIELDS]
    params = dict(model.named_parameters())
    for lens in ([300], [150, 320, 211, 64, 1, 77, 305, 256, 199, 160, 313, 240]):
        x = torch.from_numpy(np.concatenate([R.features(T, 1, D, 40 + i)[:, 0, :] for i, T in enumerate(lens)])).to(dev)
        sb = kernels.SeqBatch(lens, dev)                    # a fresh descriptor: no tables yet
        other = kernels.SeqBatch([lens[0] + 3], dev)
        xo = torch.from_numpy(R.features(lens[0] + 3, 1, D, 99)[:, 0, :]).to(dev)
        with torch.no_grad():
            ref, _ = kernels.vasnet_forward_packed(x, sb, model._params(), dict(model._opts(False), tables=None))
            assert not getattr(sb, "_vasnet_tables", None)
            a, _ = kernels.vasnet_forward_packed(x, sb, model._params(), model._opts(False))
            assert len(sb._vasnet_tables) == 1
            kernels.vasnet_forward_packed(xo, other, model._params(), model._opts(False))
            b, _ = kernels.vasnet_forward_packed(x, sb, model._params(), model._opts(False))
            assert len(sb._vasnet_tables) == 1
        assert torch.equal(ref, a) and torch.equal(ref, b)
        outs = []
        for tables in (None, "auto", "auto"):
            for p in params.values():
                p.grad = None
            opts = dict(scale=float(model.scale), eps=1e-6, ignore_self=False, aperture=None, dropout_p=0.5, seed=5, precision="fp32")
            if tables is None:
                opts["tables"] = None
            xg = x.clone().requires_grad_(True)
            s_ = VasnetFunction.apply(xg, sb, opts, None, None, names, *[params[n] for n in names])
            (s_ * torch.linspace(-1, 1, s_.numel(), device=dev)).sum().backward()
            outs.append([s_.detach().clone(), xg.grad.clone()] + [params[n].grad.clone() for n in names])
        for o in outs[1:]:
            for u, v in zip(outs[0], o):
                assert torch.equal(u, v)
