"""GPU: the Transformer-encoder scorer (csrc/transformer.hip) against the float64 functional reference oracle/torch_port.transformer_ref (plain
torch ops, run in float64 on the GPU), forward on every dispatch path and the training step at the trainer's size (D = 1024, 8 heads of 128
columns, 6 layers, F = D, ragged packed batches), with every dropout site replayed from recipes.transformer_drop_masks.

The kernel sequence is picked from the batch geometry (`regime` below restates each trigger from the source):
  GEMM tiles       128x128 when a projection has >= 512 of them, else 64x64           tf_geometry: cfg(M, N) = gemm_tiles(M, N, 0) >= 512 ? 0 : 1
  softmax form     registers for T <= 512, loops above (per video, in one launch)     tf_softmax_kernel: `if (T <= 512)`
  plane path       inference in bf16x6 / bf16x3, D, F multiples of 256, R >= 128      sumk_transformer_forward: pw = !training && npl && wplanes
                                                                                      && tf_wplanes_ok && tf_pw_rows_ok
  attention planes pw and heads of 128 columns, t_max <= 320                          tf_pw_extra: attn_pw_heads_ok (attn_pw.hip)
  in-loop split    bf16x6 / bf16x3 elsewhere (training always): launch_gemm with g.precision for every GEMM

  I1 fp32 inference, small tiles, register softmax          I2 fp32, both softmax forms, large tiles (R >= 8065)
  I3 bf16x6 / bf16x3 without planes (R < 128)               I4 planes + multi-head attention on planes (t_max = 320)
  I5 planes, attention on the in-loop kernels (T = 321; dh 256; dh 64)                 I6 the BASELINE stack in all three precisions
  T1 fp32 training step, all gradients + dx (6 layers)      T2 T1 in bf16x6 / bf16x3   T3 40 short videos
  T4 more_residuals + 'simple' table through forward(), B = 2 (table gradient)         T5 'attention' table, B = 3 (row r // B)
  T6 dropout replay (layer p 0.1, head p 0.5) in fp32 and bf16x6; another seed differs; p = 0 gives the eval-mode scores
  T7 the ReLU masks with half of every ReLU's units cut (D = 256, 2 layers), fp32 and bf16x6
The plane-path half of `regime` is also checked against the library itself (observed_paths: the workspace size it asks for).

Errors are made visible as in tests/test_gpu_vasnet_lengths.py: k2 is scaled so that the scores stay inside (0.01, 0.99) and the forward is
compared on logits recovered from the scores; the frames at tile / strip edges of each video (first / last, 63 / 64, 127 / 128, 255 / 256,
319 / 320, 511 / 512, the last 64-key block's first key and the one before) have 4x the features of the others, so a key that is dropped,
doubled or masked wrongly moves those rows by far more than the gates.

Gates come from arithmetic: the same reference run in fp32 on the same inputs (TF32 off) is the yardstick, its distance to float64.  fp32 and
bf16x6 (fp32-grade products) must stay within 4x the yardstick.  bf16x3 keeps hi + lo = 16 significant bits of each operand (representation
error <= 2^-17 relative) and drops lo x lo (<= 2^-18 |a b|), so one product carries ~2^-16 relative error where an fp32 product rounds to
2^-24: 4 x 2^8 x the yardstick.  Gradients are compared per parameter, dx per video, as norm-relative errors ||got - ref|| / ||ref|| with the
same multiples.  A gradient is compared only where no ReLU input of the float64 reference lies within a few fp32 roundings of the kink
(KINK_ULPS, asserted in ref_run): such a unit can switch sides in one fp32 run and not another.  Every training case re-runs once with every device allocation poisoned (tests/test_gpu_poison.py's Poison): bit-identical."""
import json
import math
import os

import numpy as np
import pytest
import torch

import recipes as R
from test_gpu_poison import Poison

pytestmark = pytest.mark.gpu
LIM = (1 << 31) - 65536                         # the plane kernels' 31-bit byte offsets (sumk_internal.h pw_ok, attn_pw.hip attn_pw_ok)
FP32_MULT = 4.0
BF16X3_MULT = 4.0 * 2 ** 8
NP_OF = {"bf16x6": 3, "bf16x3": 2}
# Floor of a norm-relative gradient yardstick: 4 fp32 ulps.  Storing the fp32 result alone costs up to 2^-24 relative per entry, and on a
# tensor of a few entries (k2.bias is one number) the fp32 reference can land closer to float64 than that by chance.
YARD_FLOOR = 4 * 2.0 ** -24
K2_SCALE = 1.0 / 16                             # recipes' k2 gives logits of std ~4 (saturated scores); 1/16 -> std ~0.25
RELU_SHIFT = 4.5                                # added to the linear1 / k1 biases: ReLU inputs away from the kink (make_model)
# A ReLU input whose float64 value lies within a few fp32 rounding errors of 0 may land on the other side in an fp32 run, which moves the
# gradient discretely (one unit's whole contribution) -- not an arithmetic error of either side.  The rounding error of an fp32 dot
# product is a small multiple of 2^-24 sum_k |w_k a_k| (+ |b|); a gradient case needs every ReLU input of its float64 reference at least
# KINK_ULPS of those away from 0 (a unit at 0.8 of them flipped in the HIP run and moved the layer-0 gradients by 300x the yardstick).
KINK_ULPS = 4.0


def _mult(prec):
    return BF16X3_MULT if prec == "bf16x3" else FP32_MULT


# ------------------------------------------------------------------------------------------------ the dispatch, restated from the source
def _pitch(rows):
    return (rows + 63) // 64 * 64                                                  # pw_rows_pitch


def _planes_bytes(rows, K, n):
    return _pitch(rows) * K * n * 2 + 8192                                         # pw_planes_bytes


def _alpha_bytes(rows, t_max, n):
    return _pitch(rows) * ((t_max + 31) // 32 * 32) * n * 2 + 8192                 # pw_alpha_bytes


def _pw_ok(M, N, K, a_rows, b_rows, n):                                           # sumk_internal.h pw_ok
    return M >= 1 and N % 256 == 0 and K % 32 == 0 and K >= 128 and n in (2, 3) and _planes_bytes(a_rows, K, n) < LIM and \
        _planes_bytes(b_rows, K, n) < LIM


def _tiles128(M, N):
    return -(-M // 128) * -(-N // 128)                                             # gemm_tiles(M, N, 0)


def regime(lens, D, heads, precision, training=False):
    """Which kernels csrc/transformer.hip runs for this batch (F = D, as the scorer builds it)."""
    R_, t_max, F = sum(lens), max(lens), D
    tile = lambda M, N: "large" if _tiles128(M, N) >= 512 else "small"             # tf_geometry: cfg(M, N)
    g = dict(R=R_, t_max=t_max, c_qkv=tile(R_, 3 * D), c_dd=tile(R_, D), c_df=tile(R_, F),
             softmax=sorted({"reg" if T <= 512 else "loop" for T in lens}))       # tf_softmax_kernel: if (T <= 512)
    npl = 0 if training else NP_OF.get(precision, 0)                              # sumk_transformer_forward: pw needs !training
    wplanes_ok = npl and D >= 256 and D % 256 == 0 and F % 256 == 0 and _pw_ok(256, 3 * D, D, 256, 3 * D, npl) and \
        _pw_ok(256, F, D, 256, F, npl) and _pw_ok(256, D, F, 256, D, npl)         # tf_wplanes_ok
    rows_ok = npl and R_ >= 128 and _pw_ok(R_, 3 * D, D, R_, 3 * D, npl) and _pw_ok(R_, F, D, R_, F, npl) and \
        _pw_ok(R_, D, F, R_, D, npl)                                               # tf_pw_rows_ok
    pw = bool(wplanes_ok and rows_ok)
    attn_ok = 1 <= t_max <= 320 and D % 256 == 0 and _planes_bytes(R_, 3 * D, npl or 3) < LIM       # attn_pw_ok (AP_TMAX = 320)
    heads_ok = attn_ok if heads == 1 else (heads >= 2 and D == heads * 128 and attn_ok and
                                           heads * ((_alpha_bytes(R_, t_max, npl or 3) + 255) // 256 * 256) < LIM)   # attn_pw_heads_ok
    g.update(pw=pw, pw_attn=pw and heads_ok)
    g["path"] = "pw_attn" if g["pw_attn"] else "pw_inloop" if pw else "split_inloop" if precision in NP_OF else "fp32"
    return g


def observed_paths(lens, D, heads, layers, prec, dev):
    """What the LIBRARY says about the plane path, independent of `regime`: sumk_transformer_workspace_bytes_for adds the plane buffers
    only when the plane path runs (pw), and the [Q | K | V] / alpha planes and the SeqInfo table on top only when the attention runs on
    planes too (tf_pw_extra)."""
    from summarizer_amd import _lib, kernels
    lib = _lib.load()
    sb = kernels.SeqBatch.get(lens, dev)
    size = lambda code: int(lib.sumk_transformer_workspace_bytes_for(D, D, heads, layers, sb.n_seq, sb.off_host_p, 0, code))
    base, got, n = size(0), size(kernels.precision_code(prec)), NP_OF.get(prec, 0)
    a256 = lambda v: (v + 255) // 256 * 256
    planes_only = a256(base) + 2 * a256(_planes_bytes(sum(lens), D, n)) if n else base          # tf_pw_extra: pa, pb
    return dict(pw=got != base, pw_attn=got > planes_only)


def _check_regime(cid, lens, D, heads, prec, training, expect):
    g = regime(lens, D, heads, prec, training)
    for k, v in expect.items():
        if k == "path" and (prec == "fp32") != (v == "fp32"):
            continue          # (a case named for a split-arithmetic path runs its fp32 pass on the fp32 kernels, and the other way round)
        assert g[k] == v, (cid, prec, k, g[k], v, g)
    return g


# ------------------------------------------------------------------------------------------------ inputs
def _lens_fill(head, lo, hi, min_rows, seed):
    rng = np.random.default_rng(seed)
    lens = list(head)
    while sum(lens) < min_rows:
        lens.append(int(rng.integers(lo, hi + 1)))
    return lens


def boundary_keys(T):
    ks = {0, T - 1}
    ks.update(k for k in (63, 64, 127, 128, 255, 256, 319, 320, 511, 512) if k < T)
    last = (T - 1) // 64 * 64
    ks.update(k for k in (last, last - 1) if 0 <= k < T)
    return sorted(ks)


def make_inputs(lens, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(sum(lens), D, generator=g) * 0.5
    r0 = 0
    for T in lens:
        x[[r0 + k for k in boundary_keys(T)]] *= 4.0
        r0 += T
    return x


def make_model(D, layers, heads, seed, relu_shift=None, **kw):
    from summarizer_amd.models.transformer import Transformer
    torch.manual_seed(seed)
    m = Transformer(input_size=D, encoder_layers=layers, attention_heads=heads, **kw)
    w = R.transformer_weights(D, layers, seed, max_length=kw.get("max_length") if kw.get("pos_embed", "simple") == "simple" else None)
    missing = m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not missing.unexpected_keys, missing.unexpected_keys
    with torch.no_grad():
        m.k2.weight.mul_(K2_SCALE)
        m.k2.bias.zero_()
        # ReLU inputs (linear1, k1) have std ~1.4 here; at a bias near 0, among the ~10^7 units of a 6-layer step several lie within fp32
        # rounding of the kink and switch sides in one fp32 run but not in another -- a discrete change of the gradient (a kink of the
        # function, not an error of the arithmetic).  At +4.5 (~3.2 sigma) about 0.07 % of the units are still cut and few lie near the
        # kink; ref_run asserts that none does (KINK_ULPS).  T7 covers the ReLU masks with half the units cut on a smaller stack.
        shift = RELU_SHIFT if relu_shift is None else relu_shift
        for lyr in m.transformer_encoder.layers:
            lyr.linear1.bias.add_(shift)
        m.k1.bias.add_(shift)
    return m


def _names(m):
    from summarizer_amd import kernels
    return kernels.transformer_param_names(m.encoder_layers)


# ------------------------------------------------------------------------------------------------ the float64 reference
def ref_run(m, x, lens, dtype, cw=None, masks=None, pos=None, table_key=None):
    """transformer_ref in `dtype` on x's device.  cw: back-propagate sum(cw * scores) -> (scores, logits, grads, dx per video).
    pos: (table, rows); table_key: the state_dict key of a learnable table (its gradient is returned too)."""
    from oracle import torch_port
    want = cw is not None
    sd = dict(m.named_parameters())
    keys = _names(m) + ([table_key] if table_key else [])
    p = {k: sd[k].detach().to(dtype).clone().requires_grad_(want) for k in keys}
    xs = [t.detach().to(dtype).clone().requires_grad_(want) for t in torch.split(x, lens)]
    pd = None
    if pos is not None:
        pd = (p[table_key] if table_key else pos[0].detach().to(dtype), pos[1])
    md = None
    if masks is not None:
        cv = lambda a: torch.from_numpy(a).to(device=x.device, dtype=dtype)
        md = {k: [cv(a) for a in masks[k]] for k in ("out", "ff1", "ff2")}
        md["attn"] = [[cv(a) for a in per_layer] for per_layer in masks["attn"]]
        md["head"] = cv(masks["head"])
    log = [] if want and dtype == torch.float64 else None
    with torch.set_grad_enabled(want):
        s, u = torch_port.transformer_ref(xs, p, m.encoder_layers, m.attention_heads, final_eps=float(np.float32(m.epsilon)),
                                          more_residuals=m.more_residuals, pos=pd, masks=md, relu_log=log)
    if not want:
        return s, u
    if log is not None:
        assert kink_margin(log) >= 1.0, ("a ReLU input of this case lies within KINK_ULPS fp32 roundings of the kink: its gradient "
                                         "is not a well-posed comparison -- choose other inputs", kink_margin(log))
    (s * cw.to(dtype)).sum().backward()
    return s.detach(), u.detach(), {k: v.grad for k, v in p.items()}, [t.grad for t in xs]


def kink_margin(log):
    """min over every ReLU unit of |pre-activation| / (KINK_ULPS 2^-24 sum |w a|): >= 1 when no unit may flip in an fp32 evaluation."""
    return min(float((pre.abs() / (KINK_ULPS * 2.0 ** -24 * scale)).min()) for pre, scale in log)


def _logit(s):
    s = s.double()
    return torch.log(s) - torch.log1p(-s)


def _err(s, ref_logits):
    """max |logit(s) - reference logit|; inf if s is not finite."""
    if not bool(torch.isfinite(s).all()):
        return float("inf")
    return float((_logit(s) - ref_logits).abs().max())


def _nrel(a, ref, scale=None):
    return float((a.double() - ref.double()).norm() / (scale if scale is not None else ref.double().norm()))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    prev = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32, torch.get_float32_matmul_precision())
    torch.backends.cuda.matmul.allow_tf32 = False           # the fp32 yardstick: IEEE fp32 products, no reduced-precision inputs
    torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    yield torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = prev[:2]
    torch.set_float32_matmul_precision(prev[2])


REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SUMK_TF64_REPORT")         # optional: the per-case numbers as JSON (errors, yardsticks, gates, paths)
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_scores(cid, prec, s, u64, yard, extra=None):
    assert float(_logit(s).abs().max()) < math.log(99), (cid, prec, "scores outside (0.01, 0.99)")
    err, gate = _err(s, u64), _mult(prec) * yard
    REPORT.append(dict(case=cid, precision=prec, tensor="logits", err=err, yardstick=yard, gate=gate, **(extra or {})))
    assert err <= gate, (cid, prec, err, yard, gate)


# ------------------------------------------------------------------------------------------------ inference
ALL3 = ("fp32", "bf16x6", "bf16x3")
SPLIT = ("bf16x6", "bf16x3")
INFER = {
    # id: (lens, D, heads, layers, precisions, expected {regime key: value})
    "I1_small_tiles": ([1, 2, 63, 64, 65, 200], 1024, 8, 2, ("fp32",), dict(c_qkv="small", c_dd="small", softmax=["reg"], path="fp32")),
    "I2_large_tiles_both_softmax": (_lens_fill([512, 513, 700, 1, 64], 100, 700, 8065, 1), 1024, 8, 2, ("fp32",),
                                    dict(c_qkv="large", c_dd="large", c_df="large", softmax=["loop", "reg"], path="fp32")),
    "I3_split_no_planes": ([1, 40, 70], 1024, 8, 2, ALL3, dict(R=111, pw=False, path="split_inloop")),
    "I4_planes_attn_320": (_lens_fill([320, 1, 64, 65, 255, 256, 319], 100, 320, 2000, 2), 1024, 8, 2, SPLIT, dict(t_max=320, path="pw_attn")),
    "I5_planes_t321": ([321, 1, 64, 200, 320], 1024, 8, 2, SPLIT, dict(t_max=321, path="pw_inloop")),
    "I5_planes_dh256": ([320, 1, 64, 200], 1024, 4, 2, SPLIT, dict(t_max=320, path="pw_inloop")),
    "I5_planes_dh64": ([320, 1, 64, 200], 1024, 16, 2, SPLIT, dict(t_max=320, path="pw_inloop")),
    "I6_baseline_stack": ([120, 320, 233, 64, 1, 300, 181], 1024, 8, 6, ALL3, dict(t_max=320, path="pw_attn")),
}


@pytest.mark.parametrize("cid", list(INFER))
def test_inference_paths_vs_float64(dev, monkeypatch, cid):
    lens, D, heads, layers, precs, expect = INFER[cid]
    paths = {p: _check_regime(cid, lens, D, heads, p, False, expect)["path"] for p in precs}
    for p in precs:
        g, obs = regime(lens, D, heads, p), observed_paths(lens, D, heads, layers, p, dev)
        assert obs == dict(pw=g["pw"], pw_attn=g["pw_attn"]), (cid, p, "the library's plane dispatch differs from regime()", obs, g)
    x = make_inputs(lens, D, seed=sum(lens) + heads).to(dev)
    m = make_model(D, layers, heads, 5 + layers).to(dev).eval()
    with torch.no_grad():
        s64, u64 = ref_run(m, x, lens, torch.float64)
        s32, _ = ref_run(m, x, lens, torch.float32)
    assert float(s64.min()) > 0.01 and float(s64.max()) < 0.99, (float(s64.min()), float(s64.max()))
    yard = _err(s32, u64)
    for prec in precs:
        m.precision = prec
        m._wpl = None
        with torch.no_grad():
            a = m.score_packed(x, lens).clone()
            with Poison(monkeypatch):
                m._wpl = None
                b = m.score_packed(x, lens).clone()
        assert torch.equal(_bits(a), _bits(b)), (cid, prec, "changed after the allocations were poisoned")
        _check_scores(cid, prec, a, u64, yard, dict(path=paths[prec]))


# ------------------------------------------------------------------------------------------------ training
def hip_train(m, x, lens, prec, cw, p_layer=0.0, p_head=0.0, seed=0):
    """One forward + backward through TransformerFunction (the model's autograd path) with an explicit dropout seed:
    (scores, {name: grad}, dx per video)."""
    from summarizer_amd import kernels
    from summarizer_amd.autograd import TransformerFunction
    names = _names(m)
    sd = dict(m.named_parameters())
    for q in m.parameters():
        q.grad = None
    xg = x.clone().requires_grad_(True)
    opts = dict(layer_eps=1e-5, final_eps=m.epsilon, more_residuals=m.more_residuals, precision=prec, layer_dropout_p=p_layer,
                head_dropout_p=p_head, seed=seed)
    cfg = dict(n_layers=m.encoder_layers, n_heads=m.attention_heads, dff=m.input_size)
    s = TransformerFunction.apply(xg, kernels.SeqBatch.get(lens, x.device), cfg, opts, None, None, names, *[sd[n] for n in names])
    (s * cw).sum().backward()
    return s.detach().clone(), {n: sd[n].grad.clone() for n in names}, [t.clone() for t in torch.split(xg.grad, lens)]


def _check_grads(cid, prec, got, g64, g32, dx, dx64, dx32):
    mult = _mult(prec)
    for k, ref in g64.items():
        # in_proj_bias: its key slice [D, 2D) has a mathematically zero gradient (softmax is invariant to a per-row constant), so what
        # both sides hold there is rounding noise -- the norm over the WHOLE vector is the scale it is gated against
        yard = max(_nrel(g32[k], ref), YARD_FLOOR)
        err = _nrel(got[k], ref)
        REPORT.append(dict(case=cid, precision=prec, tensor=k, err=err, yardstick=yard, gate=mult * yard))
        assert err <= mult * yard, (cid, prec, k, err, yard)
    worst = 0.0
    for i, (a, r, y) in enumerate(zip(dx, dx64, dx32)):
        yard = max(_nrel(y, r), YARD_FLOOR)
        err = _nrel(a, r)
        worst = max(worst, err / (mult * yard))
        REPORT.append(dict(case=cid, precision=prec, tensor=f"dx{i}", err=err, yardstick=yard, gate=mult * yard))
        assert err <= mult * yard, (cid, prec, f"dx video {i}", err, yard)
    REPORT.append(dict(case=cid, precision=prec, tensor="dx (worst video, err / gate)", err=worst, yardstick=None, gate=1.0))


def _cw(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(n).astype(np.float32))


T1_LENS = [1, 64, 65, 200, 321, 513]
TRAIN = {
    # id: (lens, heads, layers, precisions)
    "T1_fp32": (T1_LENS, 8, 6, ("fp32",)),
    "T2_split": (T1_LENS, 8, 6, SPLIT),
    "T3_many_short": ([int(t) for t in np.random.default_rng(40).integers(1, 71, 40)], 8, 2, ("fp32",)),
}


@pytest.mark.parametrize("cid", list(TRAIN))
def test_training_step_vs_float64_autograd(dev, monkeypatch, cid):
    lens, heads, layers, precs = TRAIN[cid]
    D = 1024
    for prec in precs:
        _check_regime(cid, lens, D, heads, prec, True, dict(path="fp32" if prec == "fp32" else "split_inloop"))
    if cid != "T3_many_short":
        assert regime(lens, D, heads, "fp32", True)["softmax"] == ["loop", "reg"]
    x = make_inputs(lens, D, seed=sum(lens)).to(dev)
    cw = _cw(sum(lens), len(lens)).to(dev)
    m = make_model(D, layers, heads, 21 + layers).to(dev).train()
    _, u64, g64, dx64 = ref_run(m, x, lens, torch.float64, cw)
    s32, _, g32, dx32 = ref_run(m, x, lens, torch.float32, cw)
    yard = _err(s32, u64)
    for prec in precs:
        s, g, dx = hip_train(m, x, lens, prec, cw)
        with Poison(monkeypatch):
            s2, g2, dx2 = hip_train(m, x, lens, prec, cw)
        assert torch.equal(_bits(s), _bits(s2)), (cid, prec, "scores changed after the allocations were poisoned")
        for k in g:
            assert torch.equal(_bits(g[k]), _bits(g2[k])), (cid, prec, k, "changed after the allocations were poisoned")
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dx, dx2)), (cid, prec, "dx changed after poisoning")
        _check_scores(cid, prec, s, u64, yard)
        _check_grads(cid, prec, g, g64, g32, dx, dx64, dx32)


@pytest.mark.parametrize("cid", ["T4_residual_simple_B2", "T5_attention_table_B3"])
def test_positional_tables_through_forward(dev, monkeypatch, cid):
    """Through Transformer.forward (x (T, B, D), grads enabled in eval mode: TransformerFunction without dropout).  T4: more_residuals,
    final eps 1e-3 and the learnable 'simple' table (row t of every batch entry; its gradient = the scatter of dx).  T5: the sinusoid
    'attention' table, whose row for packed row r = b*T + t is r // B (the reference's repeat(1, B).view(B, T, D), transformer.py:88)."""
    D, heads, layers, T = 1024, 8, 2, 150
    if cid.startswith("T4"):
        B, kw, table_key = 2, dict(more_residuals=True, max_length=200, pos_embed="simple", epsilon=1e-3), "pos_embed.weight"
    else:
        B, kw, table_key = 3, dict(max_length=200, pos_embed="attention"), None
    lens = [T] * B
    m = make_model(D, layers, heads, 31, **kw).to(dev).eval()
    xp = make_inputs(lens, D, seed=3).to(dev)                                       # packed, batch-major (seed 2 put a k1 input of T4
                                                                                    # at 0.18 of the KINK_ULPS margin)
    x = xp.view(B, T, D).permute(1, 0, 2).contiguous()
    cw = _cw(B * T, B).to(dev)
    rows = np.arange(B * T) % T if table_key else np.arange(B * T) // B
    table = m.pos_embed.weight if table_key else m.pos_embed.to(dev)
    _, u64, g64, dx64 = ref_run(m, xp, lens, torch.float64, cw, pos=(table, rows), table_key=table_key)
    s32, _, g32, dx32 = ref_run(m, xp, lens, torch.float32, cw, pos=(table, rows), table_key=table_key)

    def run():
        for q in m.parameters():
            q.grad = None
        xg = x.clone().requires_grad_(True)
        s = m(xg)                                                                   # (T, B, 1)
        sp = s[:, :, 0].t().reshape(-1)
        (sp * cw).sum().backward()
        g = {k: q.grad.clone() for k, q in m.named_parameters() if k in g64}
        return sp.detach().clone(), g, [t.clone() for t in torch.split(xg.grad.permute(1, 0, 2).reshape(B * T, D), lens)]
    s, g, dx = run()
    with Poison(monkeypatch):
        s2, g2, dx2 = run()
    assert torch.equal(_bits(s), _bits(s2)) and all(torch.equal(_bits(g[k]), _bits(g2[k])) for k in g), (cid, "poisoned re-run differs")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dx, dx2)), (cid, "dx changed after poisoning")
    assert set(g) == set(g64) and (table_key is None or table_key in g)
    _check_scores(cid, "fp32", s, u64, _err(s32, u64))
    _check_grads(cid, "fp32", g, g64, g32, dx, dx64, dx32)


@pytest.mark.parametrize("prec", ["fp32", "bf16x6"])
def test_relu_masks_half_cut_vs_float64(dev, monkeypatch, prec):
    """T7: the ReLU backward (relu_drop_bwd_kernel's mask, the k1 ReLU inside launch_ln_head_bwd) with about half of every ReLU's units cut
    (no bias shift) on a stack small enough that no unit lies near the kink (ref_run's KINK_ULPS check; model seed 41 / input seed 1
    leave the nearest at 2.9 of the margin).  All gradients and dx, poisoned re-run."""
    lens, heads, layers, D = [1, 64, 65, 130], 4, 2, 256
    x = make_inputs(lens, D, seed=1).to(dev)
    cw = _cw(sum(lens), 7).to(dev)
    m = make_model(D, layers, heads, 41, relu_shift=0.0).to(dev).train()
    with torch.no_grad():
        cut = float((torch.nn.functional.linear(x, m.transformer_encoder.layers[0].linear1.weight,
                                                 m.transformer_encoder.layers[0].linear1.bias) < 0).double().mean())
    assert 0.3 < cut < 0.7, cut
    _, u64, g64, dx64 = ref_run(m, x, lens, torch.float64, cw)
    s32, _, g32, dx32 = ref_run(m, x, lens, torch.float32, cw)
    s, g, dx = hip_train(m, x, lens, prec, cw)
    with Poison(monkeypatch):
        s2, g2, dx2 = hip_train(m, x, lens, prec, cw)
    assert torch.equal(_bits(s), _bits(s2)) and all(torch.equal(_bits(g[k]), _bits(g2[k])) for k in g), (prec, "poisoned re-run differs")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dx, dx2)), (prec, "dx changed after poisoning")
    _check_scores("T7_relu_half_cut", prec, s, u64, _err(s32, u64))
    _check_grads("T7_relu_half_cut", prec, g, g64, g32, dx, dx64, dx32)


def test_dropout_replay_vs_float64(dev, monkeypatch):
    """T6: training with dropout on (0.1 at the four sites of every layer, 0.5 after k1) at an explicit seed, against the float64 reference
    with the recipe's keep-masks at every site: scores, every gradient, dx.  Then: a second seed gives other gradients, and p = 0 gives the
    eval-mode scores -- bit for bit in fp32 (the training forward runs the inference kernels); in bf16x6 inference runs the plane path
    (other kernels, other rounding), so both sides are held to the fp32 gate against float64 instead."""
    lens, heads, layers, D = T1_LENS, 8, 6, 1024
    pl, ph, seed = 0.1, 0.5, 0x5EED1234
    x = make_inputs(lens, D, seed=sum(lens)).to(dev)
    cw = _cw(sum(lens), len(lens)).to(dev)
    m = make_model(D, layers, heads, 27).to(dev).train()
    masks = R.transformer_drop_masks(seed, pl, ph, lens, D, D, heads, layers)
    _, u64, g64, dx64 = ref_run(m, x, lens, torch.float64, cw, masks=masks)
    s32, _, g32, dx32 = ref_run(m, x, lens, torch.float32, cw, masks=masks)
    yard = _err(s32, u64)
    for prec in ("fp32", "bf16x6"):
        s, g, dx = hip_train(m, x, lens, prec, cw, pl, ph, seed)
        with Poison(monkeypatch):
            s2, g2, dx2 = hip_train(m, x, lens, prec, cw, pl, ph, seed)
        assert torch.equal(_bits(s), _bits(s2)) and all(torch.equal(_bits(g[k]), _bits(g2[k])) for k in g), (prec, "poisoned re-run differs")
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dx, dx2)), (prec, "dx changed after poisoning")
        _check_scores("T6_dropout", prec, s, u64, yard)
        _check_grads("T6_dropout", prec, g, g64, g32, dx, dx64, dx32)
        # another seed: other masks, other gradients (far outside the gate around this seed's reference)
        _, g3, _ = hip_train(m, x, lens, prec, cw, pl, ph, seed + 1)
        k = "transformer_encoder.layers.0.linear1.weight"
        assert _nrel(g3[k], g64[k]) > 100 * FP32_MULT * max(_nrel(g32[k], g64[k]), YARD_FLOOR), (prec, "a second seed drew the same masks")
    # p = 0: the training forward against eval mode
    _, u64e = ref_run(m, x, lens, torch.float64)
    s32e, _ = ref_run(m, x, lens, torch.float32)
    yard_e = _err(s32e, u64e)
    for prec in ("fp32", "bf16x6"):
        s0, _, _ = hip_train(m, x, lens, prec, cw, 0.0, 0.0, seed)
        m.eval()
        m.precision = prec
        m._wpl = None
        with torch.no_grad():
            se = m.score_packed(x, lens).clone()
        m.train()
        if prec == "fp32":
            assert torch.equal(_bits(s0), _bits(se)), "fp32: the p = 0 training forward differs from eval mode"
        else:
            assert regime(lens, D, heads, prec)["path"] == "pw_inloop"
            _check_scores("T6_p0_train", prec, s0, u64e, yard_e)
            _check_scores("T6_p0_eval", prec, se, u64e, yard_e)
