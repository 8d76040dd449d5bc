"""GPU: the SumGAN-Att stacks (csrc/tf_decoder.hip: decoder stack with cross-attention, encoder-stack entry, row scaling) against the
float64 functional references oracle/torch_port.tf_decoder_stack_ref / tf_encoder_stack_ref (plain torch ops, run in float64 on the GPU),
per video and per parameter tensor, with every dropout site replayed from recipes.tf_stack_drop_masks.

The launch sequence is picked from the batch geometry; `regime` below restates each trigger from the source and every case asserts the
values it is named for:
  K / V projection  tfd_layout: chunk = 4 layers per launch when 2D % 128 == 0 and 2D % gemm_tile_n(cfg) == 0, else 1; launch c takes
                    nl = min(chunk, L - c chunk) layers with n_group = 2D (0 when nl == 1) on 128x128 tiles when
                    gemm_tiles(R, 2 D nl, 0) >= 512, else 64x64                                          sumk_tf_decoder_forward
  layer GEMMs       128x128 when a projection has >= 512 such tiles (c_qkv, c_dd, c_df), else 64x64      tf_geometry
  softmax form      registers for T <= 512, loops above, per video                                       tf_softmax_kernel
  tnv               ceil(dh / 64) column tiles per head in the per-(video, head) tables                  tfd_cross_setup_kernel

  D1 baseline, chunk 4, T % 4 != 0        D2 D = 96: chunk 1, three K / V launches, dh = 24     D3 L = 5: launches of 4 + 1 layers
  D4 D = 400: dh = 100 (a head's last column tile lies beside the next head), chunk 1           D5 one head (tnv = 4) / 16 heads (dh = 16)
  D6 F in {64, 256, 132} at D = 128       D7 K / V launch on 128x128 tiles, layer GEMMs on 64x64, both softmax forms
  D8 every GEMM on 128x128 tiles          D1h as D1 with half of every ReLU's units cut         E1 encoder, D = 96, F = 192, with and
  without final norm                      E2 encoder on 128x128 tiles
then: dropout replay (decoder and encoder; one wrong-site run per decoder site, which must miss), null outputs, poisoned allocations,
row scaling, the model chain selector -> row scale -> encoder -> decoder, one bf16 refusal.

Inputs: tgt and memory are drawn independently; the rows at tile / strip edges of each video (boundary_keys of
tests/test_gpu_transformer_f64.py) have 4x the features of the others; norm gains and every bias are perturbed (torch starts the attention
biases at 0); the linear1 biases are shifted by RELU_SHIFT so that no ReLU input of the float64 reference lies within KINK_ULPS fp32
roundings of the kink (tests/test_gpu_transformer_f64.py; asserted on the float64 run: kink_margin >= 1), with ~0.03 % of the units cut.

Gates come from arithmetic (no fixed numbers): the same reference run in fp32 on the same inputs (TF32 off) is the yardstick, its
distance to float64.  Forward: per video, max |out - ref64| <= 4 x max |ref32 - ref64| of that video.  Gradients: norm-relative
||got - ref64|| / ||ref64||, per parameter tensor and per video for dtgt / dmemory / dx, <= 4 x max(yardstick, 4 x 2^-24).  Where a
yardstick is exactly 0 the result must equal the float64 one rounded to fp32 bit for bit.

Measured on an MI355X (worst err / gate over the tensors of a case: forward, gradients; then the kink margin of its float64 run):
  D1 0.30 0.28 5.5e3    D1h 0.28 0.29 38     D2 0.33 0.26 3.3e3    D3 0.27 0.30 2.5e4    D4 0.31 0.29 34      D5 one head 0.27 0.29 1.4e3
  D5 16 heads 0.27 0.29 561    D6 F=64 0.26 0.29 707    D6 F=256 0.27 0.29 1.1e3    D6 F=132 0.34 0.30 2.6e3    D7 0.31 0.27 6.3
  D8 0.29 0.28 6.9      E1 norm 0.32 0.27 678    E1 no norm 0.25 0.27 678    E2 0.29 0.27 11.6    dropout decoder 0.27 0.27 2.8e3
  dropout encoder 0.34 0.30 8.8e3    model chain 0.37 0.24 14 (the smallest of its four draws)    row scale ds: <= 0.06 of its gate
  (the kink margins of D7, D8 and E2 were also computed once on the CPU, where the float64 reference takes a second or two: the same)
  wrong-site runs (one decoder site's masks from seed + 1 in the reference): the kernels' result lies 1.2e5 .. 7.4e5 gates from it
  (attn 1.4e5 / 2.9e5, out 1.3e5 / 5.4e5, ff1 3.1e5 / 4.6e5, ff2 7.4e5 / 5.0e5, cattn 3.0e5 / 5.4e5, cout 1.4e5 / 4.9e5: forward /
  gradients), against the required WRONG_SITE_MISS = 100.
Nothing missed: F != D, D and dh that are no multiple of the tile, chunk = 1, the 4 + 1 split, one and 16 heads, the 128x128 tiles and
the null-output backward calls all compute what the float64 reference computes.  The file takes about 5 s; its slowest test 1.3 s.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import recipes as R
from test_gpu_poison import Poison
from test_gpu_transformer_f64 import FP32_MULT, YARD_FLOOR, _lens_fill, kink_margin, make_inputs

pytestmark = pytest.mark.gpu
RELU_SHIFT = 2.0          # linear1 inputs have std ~0.6 here (LayerNorm output times U(-1/sqrt(D), 1/sqrt(D)) weights): ~3.4 sigma
LAYER_EPS = 1e-5


# ------------------------------------------------------------------------------------------------ the dispatch, restated from the source
def _tiles128(M, N):
    return -(-M // 128) * -(-N // 128)                                             # sumk_internal.h gemm_tiles(M, N, 0)


def _tile(M, N):
    return "large" if _tiles128(M, N) >= 512 else "small"                          # cfg = gemm_tiles(M, N, 0) >= 512 ? 0 : 1


def regime(lens, D, F, heads, L):
    """Which launches csrc/tf_decoder.hip / csrc/transformer.hip run for this batch (decoder; the encoder reads c_*, softmax, tnv)."""
    R_ = sum(lens)
    N1 = 2 * D                                                                     # tfd_layout
    tile_n = 128 if _tile(R_, N1) == "large" else 64                               # gemm_tile_n(cfg)
    chunk = 4 if N1 % 128 == 0 and N1 % tile_n == 0 else 1
    n_chunks = -(-L // chunk)
    kv = []
    for c in range(n_chunks):                                                      # sumk_tf_decoder_forward: the K / V launches
        nl = min(chunk, L - c * chunk)
        kv.append(dict(nl=nl, tile=_tile(R_, 2 * D * nl), n_group=2 * D if nl > 1 else 0))
    dh = D // heads
    return dict(R=R_, chunk=chunk, n_chunks=n_chunks, kv=kv, kv_tiles=[k["tile"] for k in kv], kv_nl=[k["nl"] for k in kv],
                c_qkv=_tile(R_, 3 * D), c_dd=_tile(R_, D), c_df=_tile(R_, F),      # tf_geometry
                softmax=["reg" if T <= 512 else "loop" for T in lens],             # tf_softmax_kernel: if (T <= 512)
                dh=dh, tnv=-(-dh // 64))                                           # tfd_cross_setup_kernel / tf_setup_kernel


def _check_regime(cid, lens, D, F, heads, L, expect):
    g = regime(lens, D, F, heads, L)
    for k, v in expect.items():
        got = sorted(set(g[k])) if k == "softmax" else g[k]
        assert got == v, (cid, k, got, v, g)
    return {k: g[k] for k in ("R", "chunk", "n_chunks", "kv_tiles", "kv_nl", "c_qkv", "c_dd", "c_df", "dh", "tnv")} | \
        {"softmax": sorted(set(g["softmax"]))}


# ------------------------------------------------------------------------------------------------ inputs
def _perturb(mod, seed, relu_shift):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n.endswith("bias") or "norm" in n:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for lyr in mod.layers:
            lyr.linear1.bias.add_(relu_shift)


def make_decoder(D, F, heads, L, seed, relu_shift=RELU_SHIFT):
    """{name: fp32 CPU tensor} of a stock nn.TransformerDecoder (keys of kernels.tf_decoder_param_names('layers.', L))."""
    torch.manual_seed(seed)
    dec = nn.TransformerDecoder(nn.TransformerDecoderLayer(d_model=D, nhead=heads, dim_feedforward=F, dropout=0.0), num_layers=L)
    _perturb(dec, seed + 1, relu_shift)
    return {n: p.detach().clone() for n, p in dec.named_parameters()}


def make_encoder(D, F, heads, L, seed, norm, relu_shift=RELU_SHIFT):
    torch.manual_seed(seed)
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=D, nhead=heads, dim_feedforward=F, dropout=0.0), num_layers=L,
                                norm=nn.LayerNorm(D) if norm else None, enable_nested_tensor=False)
    _perturb(enc, seed + 1, relu_shift)
    return {n: p.detach().clone() for n, p in enc.named_parameters()}


def _G(lens, D, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((sum(lens), D)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the float64 reference / fp32 yardstick
def _dev_masks(masks, device, dtype):
    if masks is None:
        return None
    cv = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)
    return {k: [[cv(a) for a in per] if isinstance(per, list) else cv(per) for per in v] for k, v in masks.items()}


def ref_stack(kind, P, ins, lens, heads, L, dtype, G=None, masks=None, norm=False):
    """tf_decoder_stack_ref / tf_encoder_stack_ref in `dtype` on the device of the inputs.  ins: [tgt, memory] or [x], packed.
    -> dict(out, grads {name: grad}, din [[per-video grad] per input], margin (float64 only: kink_margin of the run))."""
    from oracle import torch_port
    want = G is not None
    p = {k: v.detach().to(device=ins[0].device, dtype=dtype).clone().requires_grad_(want) for k, v in P.items()}
    xs = [[v.detach().to(dtype).clone().requires_grad_(want) for v in torch.split(t, lens)] for t in ins]
    log = [] if dtype == torch.float64 else None
    md = _dev_masks(masks, ins[0].device, dtype)
    with torch.set_grad_enabled(want):
        if kind == "decoder":
            out = torch_port.tf_decoder_stack_ref(xs[0], xs[1], p, "layers.", L, heads, LAYER_EPS, masks=md, relu_log=log)
        else:
            out = torch_port.tf_encoder_stack_ref(xs[0], p, "layers.", L, heads, LAYER_EPS, final_norm="norm." if norm else None,
                                                  final_eps=LAYER_EPS, masks=md, relu_log=log)
    res = dict(out=out.detach(), margin=kink_margin(log) if log is not None else None)
    if log is not None:
        res["cut"] = float(torch.cat([(pre < 0).reshape(-1) for pre, _ in log]).double().mean())     # share of ReLU units cut
    if want:
        (out * G.to(dtype)).sum().backward()
        res.update(grads={k: v.grad for k, v in p.items()}, din=[[v.grad for v in vs] for vs in xs])
    return res


def _assert_kink(cid, r64):
    assert r64["margin"] >= 1.0, (cid, "a ReLU input of this case lies within KINK_ULPS fp32 roundings of the kink: its gradient is "
                                       "not a well-posed comparison -- choose other inputs", r64["margin"])


# ------------------------------------------------------------------------------------------------ the HIP side
def _opts(p, seed):
    o = dict(layer_eps=LAYER_EPS, final_eps=LAYER_EPS)
    if p:
        o.update(layer_dropout_p=p, seed=seed)
    return o


def hip_decoder(P, tgt, mem, lens, heads, F, L, G, p=0.0, seed=0, want_dtgt=True, want_dmemory=True):
    """Training forward + backward on the library's entries -> dict(out, grads, din [[dtgt per video] or None, [dmemory ...] or None])."""
    from summarizer_amd import kernels
    names = kernels.tf_decoder_param_names("layers.", L)
    ts = [P[n].to(tgt.device).contiguous() for n in names]
    sb = kernels.SeqBatch.get(lens, tgt.device)
    out, ws = kernels.tf_decoder_forward(tgt, mem, sb, ts, L, heads, F, _opts(p, seed), training=True)
    grads = [torch.zeros_like(t) for t in ts]
    dtgt, dmem = kernels.tf_decoder_backward(tgt, mem, sb, ts, grads, L, heads, F, _opts(p, seed), G, ws, want_dtgt=want_dtgt,
                                             want_dmemory=want_dmemory)
    torch.cuda.synchronize()
    split = lambda t: None if t is None else list(torch.split(t, lens))
    return dict(out=out, grads=dict(zip(names, grads)), din=[split(dtgt), split(dmem)])


def hip_encoder(P, x, lens, heads, F, L, G, norm, p=0.0, seed=0, want_dx=True):
    from summarizer_amd import kernels
    names = kernels.tf_encoder_param_names("layers.", L, "norm." if norm else None)
    ts = [P[n].to(x.device).contiguous() for n in names]
    sb = kernels.SeqBatch.get(lens, x.device)
    out, ws = kernels.tf_encoder_forward(x, sb, ts, L, heads, F, _opts(p, seed), training=True)
    grads = [torch.zeros_like(t) for t in ts]
    dx = kernels.tf_encoder_backward(x, sb, ts, grads, L, heads, F, _opts(p, seed), G, ws, want_dx=want_dx)
    torch.cuda.synchronize()
    return dict(out=out, grads=dict(zip(names, grads)), din=[None if dx is None else list(torch.split(dx, lens))])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    """Every tensor of result b that is present equals a's bit for bit."""
    assert torch.equal(_bits(a["out"]), _bits(b["out"])), (what, "out")
    for k in a["grads"]:
        assert torch.equal(_bits(a["grads"][k]), _bits(b["grads"][k])), (what, k)
    for i, (u, v) in enumerate(zip(a["din"], b["din"])):
        if u is not None and v is not None:
            assert all(torch.equal(_bits(s), _bits(t)) for s, t in zip(u, v)), (what, "input gradient", i)


# ------------------------------------------------------------------------------------------------ gates and report
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
    path = os.environ.get("SUMK_SGA64_REPORT")        # optional: the per-case numbers as JSON (errors, yardsticks, gates, regimes)
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)


class Gate:
    """Collects every comparison of one case (so the report holds all of them), then fails the case if any missed."""

    def __init__(self, cid, regime_=None, margin=None):
        self.cid, self.miss, self.worst = cid, [], {"forward": 0.0, "grad": 0.0}
        self.entry = dict(case=cid, regime=regime_, kink_margin=margin, tensors=[])
        REPORT.append(self.entry)

    def _put(self, kind, name, err, yard, gate, ok):
        self.entry["tensors"].append(dict(kind=kind, tensor=name, err=err, yardstick=yard, gate=gate, ok=bool(ok)))
        if gate:
            self.worst[kind] = max(self.worst[kind], err / gate)
        self.entry["worst_err_over_gate"] = dict(self.worst)
        if not ok:
            self.miss.append((kind, name, err, yard, gate))

    def check(self, kind, name, got, r64, r32):
        """kind 'forward': max-abs; 'grad': norm-relative with the floor.  A yardstick of exactly 0: bits of fp32(ref64)."""
        got64, d32 = got.double(), r32.double() - r64
        if not bool(torch.isfinite(got).all()):
            return self._put(kind, name, float("inf"), None, None, False)
        if float(d32.abs().max()) == 0.0:
            same = torch.equal(_bits(got), _bits(r64.float()))
            return self._put(kind, name, float((got64 - r64).abs().max()), 0.0, 0.0, same)
        if kind == "forward":
            err, yard = float((got64 - r64).abs().max()), float(d32.abs().max())
        else:
            scale = float(r64.norm())
            err, yard = float((got64 - r64).norm()) / scale, max(float(d32.norm()) / scale, YARD_FLOOR)
        gate = FP32_MULT * yard
        self._put(kind, name, err, yard, gate, err <= gate)

    def check_run(self, got, r64, r32, lens, in_names):
        for i, (a, b, c) in enumerate(zip(torch.split(got["out"], lens), torch.split(r64["out"], lens), torch.split(r32["out"], lens))):
            self.check("forward", f"out video {i} (T={lens[i]})", a, b, c)
        assert set(got["grads"]) == set(r64["grads"])
        for k in r64["grads"]:
            self.check("grad", k, got["grads"][k], r64["grads"][k], r32["grads"][k])
        for nm, g, a, b in zip(in_names, got["din"], r64["din"], r32["din"]):
            for i in range(len(lens)):
                self.check("grad", f"{nm} video {i} (T={lens[i]})", g[i], a[i], b[i])

    def done(self):
        assert not self.miss, (self.cid, "missed its gate", self.miss[:6], len(self.miss))


# ------------------------------------------------------------------------------------------------ decoder cases
D7_LENS = [1, 512, 513, 700, 64, 65, 100]                                          # R = 1955
D8_LENS = _lens_fill([1, 512, 513, 700], 500, 700, 8065, 8)
SMALL_KV = dict(c_qkv="small", c_dd="small", c_df="small")
DECODER = {
    # id: (D, heads, F, L, lens, relu_shift, poison, expected {regime key: value})
    "D1_baseline": (64, 4, 64, 2, [1, 2, 63, 64, 65, 130], RELU_SHIFT, False,
                    dict(chunk=4, n_chunks=1, kv_nl=[2], kv_tiles=["small"], softmax=["reg"], tnv=1, **SMALL_KV)),
    "D1h_relu_half_cut": (64, 4, 64, 2, [1, 64, 65, 130], 0.0, False, dict(chunk=4, n_chunks=1, tnv=1, **SMALL_KV)),
    "D2_chunk1_dh24": (96, 4, 96, 3, [1, 17, 65], RELU_SHIFT, True, dict(chunk=1, n_chunks=3, kv_nl=[1, 1, 1], dh=24, tnv=1, **SMALL_KV)),
    "D3_chunks_4_1": (64, 4, 64, 5, [9, 33], RELU_SHIFT, False, dict(chunk=4, n_chunks=2, kv_nl=[4, 1], **SMALL_KV)),
    "D4_dh100": (400, 4, 400, 2, [1, 64, 65, 200], RELU_SHIFT, False, dict(chunk=1, n_chunks=2, kv_nl=[1, 1], dh=100, tnv=2, **SMALL_KV)),
    "D5_one_head": (256, 1, 256, 1, [1, 70, 128], RELU_SHIFT, False, dict(dh=256, tnv=4, chunk=4, kv_nl=[1], **SMALL_KV)),
    "D5_16_heads": (256, 16, 256, 1, [1, 70, 128], RELU_SHIFT, False, dict(dh=16, tnv=1, chunk=4, kv_nl=[1], **SMALL_KV)),
    "D6_F64": (128, 4, 64, 2, [1, 40, 65], RELU_SHIFT, True, dict(chunk=4, kv_nl=[2], **SMALL_KV)),
    "D6_F256": (128, 4, 256, 2, [1, 40, 65], RELU_SHIFT, True, dict(chunk=4, kv_nl=[2], **SMALL_KV)),
    "D6_F132": (128, 4, 132, 2, [1, 40, 65], RELU_SHIFT, True, dict(chunk=4, kv_nl=[2], **SMALL_KV)),
    "D7_kv_large_tiles": (1024, 4, 1024, 2, D7_LENS, RELU_SHIFT, False,
                          dict(chunk=4, n_chunks=1, kv_nl=[2], kv_tiles=["large"], softmax=["loop", "reg"], dh=256, tnv=4, **SMALL_KV)),
    "D8_all_large_tiles": (1024, 4, 1024, 1, D8_LENS, RELU_SHIFT, False,
                           dict(chunk=4, n_chunks=1, kv_nl=[1], kv_tiles=["large"], c_qkv="large", c_dd="large", c_df="large",
                                softmax=["loop", "reg"])),
}


def _decoder_case(cid):
    D, heads, F, L, lens, shift, poison, expect = DECODER[cid]
    seed = sum(ord(c) for c in cid)
    P = make_decoder(D, F, heads, L, seed, shift)
    return D, heads, F, L, lens, poison, expect, P, make_inputs(lens, D, seed + 2), make_inputs(lens, D, seed + 3), _G(lens, D, seed + 4)


@pytest.mark.parametrize("cid", list(DECODER))
def test_decoder_stack_vs_float64(dev, monkeypatch, cid):
    from summarizer_amd import kernels
    D, heads, F, L, lens, poison, expect, P, tgt, mem, G = _decoder_case(cid)
    g = _check_regime(cid, lens, D, F, heads, L, expect)
    assert 1921 <= g["R"] <= 8064 if cid.startswith("D7") else g["R"] >= 8065 if cid.startswith("D8") else True
    tgt, mem, G = tgt.to(dev), mem.to(dev), G.to(dev)
    r64 = ref_stack("decoder", P, [tgt, mem], lens, heads, L, torch.float64, G)
    _assert_kink(cid, r64)
    if cid.startswith("D1h"):
        assert 0.3 < r64["cut"] < 0.7, r64["cut"]
    r32 = ref_stack("decoder", P, [tgt, mem], lens, heads, L, torch.float32, G)
    got = hip_decoder(P, tgt, mem, lens, heads, F, L, G)
    if poison:
        with Poison(monkeypatch):
            kernels._ws_cache.clear()
            _same_bits(got, hip_decoder(P, tgt, mem, lens, heads, F, L, G), (cid, "poisoned allocations"))
    gate = Gate(cid, g, r64["margin"])
    gate.check_run(got, r64, r32, lens, ["dtgt", "dmemory"])
    gate.done()


# ------------------------------------------------------------------------------------------------ encoder cases
ENCODER = {
    # id: (D, heads, F, L, lens, final norm, expected regime)
    "E1_F192_final_norm": (96, 4, 192, 2, [1, 17, 65], True, dict(dh=24, tnv=1, **SMALL_KV)),
    "E1_F192_no_norm": (96, 4, 192, 2, [1, 17, 65], False, dict(dh=24, tnv=1, **SMALL_KV)),
    "E2_large_tiles": (1024, 4, 1024, 1, D8_LENS, False, dict(c_qkv="large", c_dd="large", c_df="large", softmax=["loop", "reg"])),
}


@pytest.mark.parametrize("cid", list(ENCODER))
def test_encoder_stack_vs_float64(dev, cid):
    D, heads, F, L, lens, norm, expect = ENCODER[cid]
    g = _check_regime(cid, lens, D, F, heads, L, expect)
    assert g["R"] >= 8065 if cid.startswith("E2") else True
    seed = sum(ord(c) for c in cid[:2])
    P = make_encoder(D, F, heads, L, seed, norm)
    x, G = make_inputs(lens, D, seed + 2).to(dev), _G(lens, D, seed + 4).to(dev)
    r64 = ref_stack("encoder", P, [x], lens, heads, L, torch.float64, G, norm=norm)
    _assert_kink(cid, r64)
    r32 = ref_stack("encoder", P, [x], lens, heads, L, torch.float32, G, norm=norm)
    got = hip_encoder(P, x, lens, heads, F, L, G, norm)
    gate = Gate(cid, g, r64["margin"])
    gate.check_run(got, r64, r32, lens, ["dx"])
    gate.done()


# ------------------------------------------------------------------------------------------------ dropout replay
DROP = dict(D=128, heads=4, F=128, L=2, lens=[1, 65, 200], p=0.1, seed=0x5EED4321)
DECODER_SITES = ("attn", "out", "ff1", "ff2", "cattn", "cout")
# A site's masks from another seed differ at ~2 p (1 - p) = 18 % of its elements, each an O(1) relative change of that element, while a
# gate is a few fp32 roundings (~1e-6 relative): such a reference is ~1e5 gates away.  Required: at least this many.
WRONG_SITE_MISS = 100.0


def test_decoder_dropout_replay_vs_float64(dev):
    """Training with dropout 0.1 at the six sites of every decoder layer at an explicit seed, against the float64 reference with the
    recipe's keep-masks at every site: outputs, every gradient, dtgt and dmemory per video.  Then a reference in which ONE site's masks
    (all layers) come from another seed: the kernels' result must miss that reference by a wide margin at every site -- a backward (or
    forward) that drew a site's mask with another site number or another index would show the same way.  Measured: see RESULTS."""
    from summarizer_amd import kernels
    c = DROP
    D, heads, F, L, lens, p, seed = c["D"], c["heads"], c["F"], c["L"], c["lens"], c["p"], c["seed"]
    P = make_decoder(D, F, heads, L, 77)
    tgt, mem, G = make_inputs(lens, D, 78).to(dev), make_inputs(lens, D, 79).to(dev), _G(lens, D, 80).to(dev)
    masks = R.tf_stack_drop_masks(seed, p, lens, D, F, heads, L, decoder=True)
    r64 = ref_stack("decoder", P, [tgt, mem], lens, heads, L, torch.float64, G, masks=masks)
    _assert_kink("dropout_decoder", r64)
    r32 = ref_stack("decoder", P, [tgt, mem], lens, heads, L, torch.float32, G, masks=masks)
    got = hip_decoder(P, tgt, mem, lens, heads, F, L, G, p, seed)
    gate = Gate("dropout_decoder", _check_regime("dropout_decoder", lens, D, F, heads, L, dict(chunk=4, kv_nl=[2])), r64["margin"])
    gate.check_run(got, r64, r32, lens, ["dtgt", "dmemory"])
    # another seed: other masks, another result
    other = hip_decoder(P, tgt, mem, lens, heads, F, L, G, p, seed + 1)
    assert not torch.equal(got["out"], other["out"]) and not torch.equal(got["grads"]["layers.0.linear1.weight"], other["grads"]["layers.0.linear1.weight"])
    # p = 0 in training mode: the inference forward's output, bit for bit
    names = kernels.tf_decoder_param_names("layers.", L)
    ts = [P[n].to(dev).contiguous() for n in names]
    sb = kernels.SeqBatch.get(lens, dev)
    ev, _ = kernels.tf_decoder_forward(tgt, mem, sb, ts, L, heads, F, _opts(0.0, 0), training=False)
    assert torch.equal(_bits(hip_decoder(P, tgt, mem, lens, heads, F, L, G)["out"]), _bits(ev.clone()))
    gate.done()
    # one wrong site at a time
    masks2 = R.tf_stack_drop_masks(seed + 1, p, lens, D, F, heads, L, decoder=True)
    for site in DECODER_SITES:
        wrong = dict(masks, **{site: masks2[site]})
        w64 = ref_stack("decoder", P, [tgt, mem], lens, heads, L, torch.float64, G, masks=wrong)
        w32 = ref_stack("decoder", P, [tgt, mem], lens, heads, L, torch.float32, G, masks=wrong)
        probe = Gate(f"dropout_decoder_wrong_site_{site}")
        probe.check_run(got, w64, w32, lens, ["dtgt", "dmemory"])
        worst = max(probe.worst.values())
        probe.entry["expected"] = "miss"
        assert probe.miss and worst >= WRONG_SITE_MISS, (site, "the test cannot tell this site's masks from another seed's", worst)


def test_encoder_dropout_replay_vs_float64(dev):
    from summarizer_amd import kernels
    c = DROP
    D, heads, F, L, lens, p, seed = c["D"], c["heads"], c["F"], c["L"], c["lens"], c["p"], c["seed"]
    P = make_encoder(D, F, heads, L, 87, True)
    x, G = make_inputs(lens, D, 88).to(dev), _G(lens, D, 89).to(dev)
    masks = R.tf_stack_drop_masks(seed, p, lens, D, F, heads, L, decoder=False)
    r64 = ref_stack("encoder", P, [x], lens, heads, L, torch.float64, G, masks=masks, norm=True)
    _assert_kink("dropout_encoder", r64)
    r32 = ref_stack("encoder", P, [x], lens, heads, L, torch.float32, G, masks=masks, norm=True)
    got = hip_encoder(P, x, lens, heads, F, L, G, True, p, seed)
    gate = Gate("dropout_encoder", _check_regime("dropout_encoder", lens, D, F, heads, L, {}), r64["margin"])
    gate.check_run(got, r64, r32, lens, ["dx"])
    other = hip_encoder(P, x, lens, heads, F, L, G, True, p, seed + 1)
    assert not torch.equal(got["out"], other["out"]) and not torch.equal(got["grads"]["layers.0.linear1.weight"], other["grads"]["layers.0.linear1.weight"])
    names = kernels.tf_encoder_param_names("layers.", L, "norm.")
    ts = [P[n].to(dev).contiguous() for n in names]
    ev, _ = kernels.tf_encoder_forward(x, kernels.SeqBatch.get(lens, dev), ts, L, heads, F, _opts(0.0, 0), training=False)
    assert torch.equal(_bits(hip_encoder(P, x, lens, heads, F, L, G, True)["out"]), _bits(ev.clone()))
    gate.done()


# ------------------------------------------------------------------------------------------------ null outputs
def test_null_output_backward_paths(dev):
    """sumk_tf_decoder_backward without dmemory (no dMemory GEMM), without dtgt, without both, and sumk_tf_encoder_backward without dx:
    every output still produced is bit-identical to the full call's."""
    D, heads, F, L, lens, _, _, P, tgt, mem, G = _decoder_case("D1_baseline")
    tgt, mem, G = tgt.to(dev), mem.to(dev), G.to(dev)
    full = hip_decoder(P, tgt, mem, lens, heads, F, L, G)
    for want_dtgt, want_dmem in ((True, False), (False, True), (False, False)):
        part = hip_decoder(P, tgt, mem, lens, heads, F, L, G, want_dtgt=want_dtgt, want_dmemory=want_dmem)
        assert (part["din"][0] is not None) == want_dtgt and (part["din"][1] is not None) == want_dmem
        _same_bits(full, part, ("decoder", want_dtgt, want_dmem))
    PE = make_encoder(D, F, heads, L, 5, True)
    full = hip_encoder(PE, tgt, lens, heads, F, L, G, True)
    part = hip_encoder(PE, tgt, lens, heads, F, L, G, True, want_dx=False)
    assert part["din"][0] is None and full["din"][0] is not None
    _same_bits(full, part, "encoder without dx")


def test_bf16_precisions_are_refused(dev):
    from summarizer_amd import kernels
    from summarizer_amd._lib import SumkError
    D, heads, F, L, lens, _, _, P, tgt, mem, _ = _decoder_case("D1_baseline")
    ts = [P[n].to(dev).contiguous() for n in kernels.tf_decoder_param_names("layers.", L)]
    with pytest.raises(SumkError):
        kernels.tf_decoder_forward(tgt.to(dev), mem.to(dev), kernels.SeqBatch.get(lens, dev), ts, L, heads, F,
                                   dict(layer_eps=LAYER_EPS, precision="bf16x6"), training=True)


# ------------------------------------------------------------------------------------------------ row scaling
def _dot_kernel_order(x, g):
    """<x_r, g_r> in fp32 as row_scale_bwd_kernel sums it: lane = float4 index % 64 walks its float4s in order, four products added
    left to right per float4, then the xor-shuffle butterfly over the 64 lanes (offsets 32, 16, .. 1).  numpy, fp32 throughout."""
    n, D = x.shape
    d4 = D // 4
    prod = (x.astype(np.float32) * g.astype(np.float32)).reshape(n, d4, 4)
    lanes = np.zeros((n, 64), np.float32)
    for c in range(d4):
        q = prod[:, c]
        lanes[:, c % 64] = lanes[:, c % 64] + (((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3])
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(64) ^ o]
        o >>= 1
    return lanes[:, 0]


@pytest.mark.parametrize("n_rows,D", [(1, 4), (3, 64), (5, 256), (301, 1000), (7, 1024)])
def test_row_scale_vs_float64(dev, n_rows, D):
    """y = x s and dx = s g are single fp32 products: the float64 product rounded to fp32, bit for bit.  ds = <x, g> per row against
    float64; yardstick: the same dot product summed in fp32 in the kernel's order (_dot_kernel_order).  The rounding error of a dot
    product is bounded relative to sum |x g|, not to the (possibly cancelling) sum, so that is the scale of error and floor alike.
    d4 = D / 4 float4s per row: below 64 (lanes without work), a multiple of 64, and 250 (the last pass of the loop is partial)."""
    from summarizer_amd import kernels
    rng = np.random.default_rng(n_rows * 10007 + D)
    x, s, g = (rng.standard_normal(sh).astype(np.float32) for sh in ((n_rows, D), (n_rows,), (n_rows, D)))
    xd, sd, gd = (torch.from_numpy(a).to(dev) for a in (x, s, g))
    y = kernels.row_scale_forward(xd, sd)
    dx, ds = kernels.row_scale_backward(xd, sd, gd)
    assert torch.equal(_bits(y), _bits((xd.double() * sd.double()[:, None]).float())), "y"
    assert torch.equal(_bits(dx), _bits((gd.double() * sd.double()[:, None]).float())), "dx"
    ds64 = (x.astype(np.float64) * g.astype(np.float64)).sum(1)
    scale = float(np.linalg.norm(np.abs(x.astype(np.float64) * g.astype(np.float64)).sum(1)))
    err = float(np.linalg.norm(ds.double().cpu().numpy() - ds64)) / scale
    yard = max(float(np.linalg.norm(_dot_kernel_order(x, g).astype(np.float64) - ds64)) / scale, YARD_FLOOR)
    REPORT.append(dict(case=f"row_scale_{n_rows}x{D}", tensors=[dict(kind="grad", tensor="ds", err=err, yardstick=yard, gate=FP32_MULT * yard)]))
    assert err <= FP32_MULT * yard, (err, yard)
    dx1, none = kernels.row_scale_backward(xd, sd, gd, want_ds=False)
    none2, ds1 = kernels.row_scale_backward(xd, sd, gd, want_dx=False)
    assert none is None and none2 is None
    assert torch.equal(_bits(dx1), _bits(dx)) and torch.equal(_bits(ds1), _bits(ds))


# ------------------------------------------------------------------------------------------------ the model chain
def _stock_chain(summ, x, G1, G2, log=None):
    """selector -> x * scores -> autoencoder's encoder -> decoder through the stock modules SumGANAtt holds; x (T, 1, D)."""
    hooks = []
    if log is not None:
        def hook(mod, inp, out):
            a = inp[0].detach().reshape(-1, inp[0].shape[-1])
            log.append((out.detach().reshape(a.shape[0], -1), torch.nn.functional.linear(a.abs(), mod.weight.detach().abs(), mod.bias.detach().abs())))
        for stack in (summ.selector.transformer_encoder, summ.ae.transformer_encoder, summ.ae.transformer_decoder):
            hooks += [lyr.linear1.register_forward_hook(hook) for lyr in stack.layers]
    for q in summ.parameters():
        q.grad = None
    scores = summ.selector.out(summ.selector.transformer_encoder(x))
    xw = x * scores
    x_hat = summ.ae.transformer_decoder(xw, summ.ae.transformer_encoder(xw))
    ((x_hat * G1).sum() + (scores * G2).sum()).backward()
    for h in hooks:
        h.remove()
    return x_hat.detach(), scores.detach(), {n: q.grad.clone() for n, q in summ.named_parameters() if q.grad is not None}


CHAIN_DRAWS = (72, 73, 74, 75)


def _chain_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(40, 1, 64, generator=g), torch.randn(40, 1, 64, generator=g), torch.randn(40, 1, 1, generator=g)


def _chain_model():
    from summarizer_amd.models.sumgan_att import SumGANAtt
    torch.manual_seed(71)
    m = SumGANAtt(input_size=64, s_encoder_layers=2, s_attention_heads=4, ae_encoder_layers=2, ae_attention_heads=4,
                  cLSTM_hidden_size=32, cLSTM_num_layers=2).train()
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, nn.MultiheadAttention):
            mod.dropout = 0.0
    return m


def test_model_chain_gradients_vs_float64(dev):
    """test_model_classes_vs_stock_modules' setting (tests/test_gpu_sumgan_att.py: input 64, 2 + 2 layers, 4 heads, 40 frames, .train() with
    every dropout p at 0): gradients of (x_hat * G1).sum() + (scores * G2).sum() for every used parameter through the HIP chain
    selector -> row scale -> encoder -> decoder, against the float64 stock modules the model holds; yardstick: the same modules in fp32.

    The chain is run on CHAIN_DRAWS independent draws of (x, G1, G2).  x_hat and scores are gated per draw; a parameter's gradient is
    gated as ONE tensor holding its gradients of all draws side by side.  Why not draw by draw: selector.out.0.bias is one number, a
    sum over the 40 rows of du = dscores * s (1 - s) that cancels to ~0.4 of its rms, and every bias of the selector (column sums of a
    stream that is du times a fixed row) inherits it.  The error of such a sum is ONE random draw on either side: over six draws the
    fp32 stock chain's error on it ranged 6.1e-7 .. 6.6e-6 and the kernels' 4.1e-7 .. 2.7e-6, while the stream gradients feeding
    the sum (d scores, d hidden) were within 0.67 .. 1.12 of the yardstick in every draw.  At draw 72 alone the yardstick drew low
    (6.3e-7) and the kernels high (2.7e-6): 1.07 gates on out.0.bias, 1.01 on layers.1.norm2.bias -- a property of a one-number
    yardstick, not of the arithmetic (the scorer's test floors its yardsticks for the same reason)."""
    import copy
    m = _chain_model()
    s64, s32 = copy.deepcopy(m.summarizer).double().to(dev), copy.deepcopy(m.summarizer).to(dev)
    m = m.to(dev)
    params = dict(m.summarizer.named_parameters())
    used = [n for n in params if "_layer." not in n]
    gate = Gate("model_chain", None, None)
    got, r64, r32, margins = {n: [] for n in used}, {n: [] for n in used}, {n: [] for n in used}, []
    for seed in CHAIN_DRAWS:
        x, G1, G2 = (t.to(dev) for t in _chain_inputs(seed))
        log = []
        xh64, sc64, g64 = _stock_chain(s64, x.double(), G1.double(), G2.double(), log)
        margins.append(kink_margin(log))
        assert margins[-1] >= 1.0, ("a ReLU input lies within KINK_ULPS fp32 roundings of the kink -- choose other inputs", seed, margins[-1])
        xh32, sc32, g32 = _stock_chain(s32, x, G1, G2)
        for q in m.summarizer.parameters():
            q.grad = None
        x_hat, scores = m.summarizer(x)
        ((x_hat * G1).sum() + (scores * G2).sum()).backward()
        assert sorted(used) == sorted(g64)
        gate.check("forward", f"x_hat draw {seed}", x_hat.detach().reshape(40, 64), xh64.reshape(40, 64), xh32.reshape(40, 64))
        gate.check("forward", f"scores draw {seed}", scores.detach().reshape(40), sc64.reshape(40), sc32.reshape(40))
        for n in used:
            assert params[n].grad is not None, n
            got[n].append(params[n].grad.reshape(-1).clone()); r64[n].append(g64[n].reshape(-1)); r32[n].append(g32[n].reshape(-1))
    gate.entry["kink_margin"] = min(margins)
    for n in used:
        gate.check("grad", n, torch.cat(got[n]), torch.cat(r64[n]), torch.cat(r32[n]))
    gate.done()
