"""Host-side checks of the bf16x3 streaming attention's test infrastructure and host arithmetic (no GPU):
  * tests/attn_stream_split_ref.py: its split is oracle/torch_port.split_bf16 bit for bit, and with float64 accumulation it is
    oracle/torch_port.mm3 applied to the dense formula;
  * the families of tests/attn_stream_split_cases.py: the x3 yardstick of each is at most 4 x 2^8 fp32 yardsticks (BF16X3_MULT, the bound
    tests/test_gpu_vasnet_lengths.py derives) -- a condition on the INPUTS that keeps a blown-up yardstick from hiding a kernel error;
  * the gate of tests/test_gpu_attn_stream_split.py discriminates: the specification passes its own worst() in every family, and each
    mutant (a dropped plane product in either product, a one-plane P, a V fragment in natural key order, a lost key of the partial last
    tile) fails it in at least one strips family;
  * the workspace queries answer without a GPU and grow as the header states; the profiler tags match the header."""
import os
import re

import numpy as np
import pytest
import torch

import attn_stream_cases as base
import attn_stream_split_cases as cases
import attn_stream_split_ref as ref
from oracle import torch_port
from test_gpu_attn_stream_split import worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_is_torch_ports():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(200000) * np.exp(rng.uniform(-30, 30, 200000))).astype(np.float32)
    x[:8] = [0.0, -0.0, 1.0, 1.00390625, 1.01171875, np.float32(2.0 ** -126), np.float32(3.3895314e38), np.float32(1e-40)]   # ties, the edges
    hi, lo = ref.split(x)
    thi, tlo = torch_port.split_bf16(torch.from_numpy(x))
    assert np.array_equal(hi.view(np.uint32), thi.numpy().view(np.uint32))
    assert np.array_equal(lo.view(np.uint32), tlo.numpy().view(np.uint32))
    assert not (hi.view(np.uint32) & 0xFFFF).any() and not (lo.view(np.uint32) & 0xFFFF).any()
    n = ref.split(np.array([np.nan, 1.0], dtype=np.float32))
    assert np.isnan(n[0][0]) and np.isnan(n[1][0]) and n[0][1] == 1.0 and n[1][1] == 0.0


def _dense_mm3(c):
    """The dense formula with oracle/torch_port.mm3 for both products, in float64."""
    sc = base.scale_of(c)
    Q, K, V = (torch.from_numpy(c[n]).double() for n in "qkv")
    D, heads = c["D"], c["heads"]
    dh = D // heads
    ctx = torch.zeros(Q.shape[0], D, dtype=torch.float64)
    lse = torch.zeros(Q.shape[0], heads, dtype=torch.float64)
    r0 = 0
    for T in c["lens"]:
        for h in range(heads):
            q, k, v = (a[r0:r0 + T, h * dh:(h + 1) * dh] for a in (Q, K, V))
            s = torch_port.mm3(q, k.t()).float()                    # the logits leave the accumulator as float32
            e = s * np.float32(sc)
            m = e.max(dim=1, keepdim=True).values
            p = torch.exp(e - m)
            tot = p.sum(dim=1, keepdim=True)
            ctx[r0:r0 + T, h * dh:(h + 1) * dh] = (torch_port.mm3(p.double(), v).float() / tot).double()
            lse[r0:r0 + T, h] = (m + torch.log(tot))[:, 0].double()
        r0 += T
    return ctx.numpy(), lse.numpy()


@pytest.mark.parametrize("D,heads,T", ((32, 4, 65), (80, 2, 129), (256, 2, 200)))
def test_float64_accumulation_is_mm3(D, heads, T):
    """mha3 with float64 accumulators = the dense formula on torch_port.mm3: the same planes, the same three products, lo.lo dropped.  What
    is left between them is float32 rounding in two libraries: exp (1 ulp each), the row sum in another order (log2 T ulps), the division,
    and a logit that the two float64 summation orders round to neighbouring floats (1 ulp of |e| <= 64 moves a weight by 64 ulps at most,
    a row of ctx by less) -- 64 ulps of the largest element bounds them; a dropped plane product is 2^-9, the arithmetic itself 2^-17."""
    c = base.case(f"mm3_T{T}_D{D}", (T,), D, heads, 17 + T)
    ctx, lse = ref.mha3(c["q"], c["k"], c["v"], c["lens"], heads, base.scale_of(c), acc=np.float64)
    rc, rl = _dense_mm3(c)
    tol = 64 * 2.0 ** -24
    dc, dl = np.abs(ctx - rc).max() / np.abs(rc).max(), np.abs(lse - rl).max() / np.abs(rl).max()
    print(f"T{T} D{D}: ctx {dc / 2.0 ** -24:.1f} ulps, lse {dl / 2.0 ** -24:.1f} ulps of the largest element")
    assert dc <= tol and dl <= tol, (dc, dl)
    for mutant in ("first_no_lohi", "second_no_hilo", "p_one_plane"):          # ... and a missing plane product is far outside it
        mc, _ = ref.mha3(c["q"], c["k"], c["v"], c["lens"], heads, base.scale_of(c), acc=np.float64, mutant=mutant)
        assert np.abs(mc - rc).max() / np.abs(rc).max() > 4 * tol, mutant


@pytest.mark.parametrize("name", sorted(cases.families()))
def test_x3_yardstick_within_bound_and_spec_passes(name):
    fam = cases.families()[name]
    yc3, yl3, yc32, yl32 = cases.yardsticks(fam)
    print(f"{name}: x3 yardsticks ctx {yc3:.3e} lse {yl3:.3e}; fp32 ctx {yc32:.3e} lse {yl32:.3e}; ratios {yc3 / yc32:.1f} {yl3 / yl32:.1f}")
    assert 0 < yc3 <= cases.BF16X3_MULT * yc32, (name, yc3, yc32)
    assert 0 < yl3 <= cases.BF16X3_MULT * yl32, (name, yl3, yl32)
    for c in fam:                                            # the specification itself is inside the gate, by construction at most 1
        s = cases.spec(c)
        assert worst(s[4], s[0], yc3, (c["name"], "ctx")) <= 1.0 and worst(s[5], s[1], yl3, (c["name"], "lse")) <= 1.0


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_gate_catches(mutant):
    """Each wrong kernel fails the GPU test's own worst() in at least one strips family (the search stops at the first case that fails)."""
    for D, heads in cases.STRIP_SHAPES:
        fam = cases.strips(D, heads)
        yc, yl = cases.yardsticks(fam)[:2]
        for c in reversed(fam):                              # long videos first: more tiles, partial last tiles
            ctx, lse = ref.mha3(c["q"], c["k"], c["v"], c["lens"], heads, base.scale_of(c), mutant=mutant)
            try:
                worst(ctx, cases.spec(c)[0], yc, (c["name"], "ctx"))
                worst(lse, cases.spec(c)[1], yl, (c["name"], "lse"))
            except AssertionError as e:
                print(f"{mutant}: caught at {c['name']}: {e.args[0]}")
                return
    pytest.fail(f"the gate lets the mutant {mutant} through every strips family")


def test_workspace_queries_and_tags():
    from summarizer_amd import _lib
    lib = _lib.load()
    X3 = 1

    def ws(D, heads, lens, prec=X3):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        return int(lib.sumk_attn_stream_split_workspace_bytes(D, heads, len(lens), _lib.host_i32(off), prec))

    def tf(D, heads, lens, prec=X3, layers=6, split=True):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        if split:
            return int(lib.sumk_transformer_stream_split_workspace_bytes(D, D, heads, layers, len(lens), _lib.host_i32(off), prec))
        return int(lib.sumk_transformer_stream_workspace_bytes(D, D, heads, layers, len(lens), _lib.host_i32(off)))

    up = lambda b: (b + 255) // 256 * 256
    # descriptors (24 bytes per video) + three plane blocks of heads x padded rows x staged columns x 4 bytes
    assert ws(1024, 8, [64]) == 256 + 3 * 8 * 64 * 128 * 4
    assert ws(1024, 8, [1]) == ws(1024, 8, [64]) and ws(1024, 8, [65]) == 256 + 3 * 8 * 128 * 128 * 4        # videos padded to 64-key tiles
    assert ws(1024, 8, [65, 1, 64]) == 256 + 3 * 8 * 256 * 128 * 4                                           # ... each on its own
    assert ws(80, 2, [64]) == 256 + 3 * 2 * 64 * 64 * 4 and ws(208, 2, [64]) == 256 + 3 * 2 * 64 * 128 * 4   # dh 40 -> 64, 104 -> 128 columns
    assert ws(32, 4, [64]) == 256 + 3 * 4 * 64 * 32 * 4
    assert ws(1024, 8, [64] * 20) == up(24 * 20) + 3 * 8 * 64 * 20 * 128 * 4
    assert ws(1024, 8, [65536]) == 256 + 3 * 65536 * 1024 * 4                                               # 4 bytes per element and operand
    for bad in ((8, 2, [10]), (72, 2, [10]), (512, 2, [10]), (64, 3, [10]), (64, 2, [10, 0]), (64, 2, [1 << 20]), (64, 2, [])):
        assert ws(*bad) == 0, bad
    for prec in (0, 2, 3, 7, -1):
        assert ws(64, 2, [10], prec) == 0 and f"precision={prec}".encode() in lib.sumk_last_error(), prec
        assert tf(64, 2, [10], prec) == 0
    assert ws(8, 2, [10]) == 0 and b"head width 4" in lib.sumk_last_error()
    assert ws(512, 2, [10]) == 0 and b"head width 256" in lib.sumk_last_error()
    # the transformer carve: the stream carve + the planes of one layer, whatever the number of layers
    for lens in ([200, 65], [8192]):
        for layers in (1, 6):
            assert tf(1024, 8, lens, layers=layers) == tf(1024, 8, lens, layers=layers, split=False) + ws(1024, 8, lens)
    src = open(os.path.join(ROOT, "include", "sumk.h")).read()
    tags = {k: int(v) for k, v in re.findall(r"#define (SUMK_PROF_[A-Z0-9_]+) (\d+)", src)}
    assert tags["SUMK_PROF_ATTN_STREAM_SPLIT_PLANES"] == _lib.PROF_ATTN_STREAM_SPLIT_PLANES < _lib.PROF_NTAGS
    assert tags["SUMK_PROF_ATTN_STREAM_SPLIT"] == _lib.PROF_ATTN_STREAM_SPLIT < _lib.PROF_NTAGS == tags["SUMK_PROF_NTAGS"] <= 32


def test_python_arguments_without_a_gpu():
    from summarizer_amd import kernels
    from summarizer_amd._lib import SumkError
    from summarizer_amd.models.transformer import Transformer
    sb = kernels.SeqBatch.get([200, 65], torch.device("cpu"))
    a = kernels.attn_stream_workspace_bytes(1024, 8, sb)
    assert a == kernels.attn_stream_workspace_bytes(1024, 8, sb, precision="fp32") == 256
    assert kernels.attn_stream_workspace_bytes(1024, 8, sb, precision="bf16x3") == 256 + 3 * (256 + 128) * 1024 * 4
    t = kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream")
    assert t == kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", attention_precision="fp32")
    assert kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", attention_precision="bf16x3") == t + 256 + 3 * 384 * 1024 * 4
    for bad in ("bf16x6", "bf16", "fp16"):
        with pytest.raises(SumkError):
            kernels.attn_stream_workspace_bytes(1024, 8, sb, precision=bad)
        with pytest.raises(SumkError):
            kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", attention_precision=bad)
    with pytest.raises(SumkError):
        kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "dense", attention_precision="bf16x3")
    with pytest.raises(SumkError):
        kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", training=True, attention_precision="bf16x3")
    with pytest.raises(ValueError, match="attention_precision"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention="stream", attention_precision="bf16x6")
    with pytest.raises(ValueError, match="attention='stream'"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention="dense", attention_precision="bf16x3")
    m = Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention="stream", attention_precision="bf16x3")
    assert m.attention_precision == "bf16x3"
    assert Transformer(input_size=64, encoder_layers=1, attention_heads=2).attention_precision == "fp32"


def test_trainer_takes_attention_precision():
    from summarizer_amd.models.transformer import TransformerTrainer

    class _Hps:
        extra_params = {"input_size": "64", "encoder_layers": "1", "attention_heads": "2", "attention": "stream", "attention_precision": "bf16x3"}
        use_cuda = False
    t = TransformerTrainer.__new__(TransformerTrainer)
    t.hps = _Hps()
    m = t._init_model()
    assert m.attention == "stream" and m.attention_precision == "bf16x3" and m.precision == "fp32"
    _Hps.extra_params = {"input_size": "64", "encoder_layers": "1", "attention_heads": "2", "attention": "stream"}
    assert t._init_model().attention_precision == "fp32"
    _Hps.extra_params = {"input_size": "64", "encoder_layers": "1", "attention_heads": "2", "attention_precision": "bf16x3"}
    with pytest.raises(ValueError, match="needs attention='stream'"):
        t._init_model()
