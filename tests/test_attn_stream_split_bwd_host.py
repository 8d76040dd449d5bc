"""Host-side checks of the bf16x3 streaming attention's training form and backward: test infrastructure and host arithmetic (no GPU).
  * the families of tests/attn_stream_split_bwd_cases.py: per family and per output (ctx, dQ, dK, dV) the bf16x3 yardstick is at most 4 x 2^8
    fp32 yardsticks (BF16X3_MULT) -- a condition on the INPUTS that keeps a blown-up yardstick from hiding a kernel error -- and the
    specification itself passes the GPU test's gate with ratio at most 1;
  * tests/attn_stream_split_bwd_ref.py with float64 accumulation is the dense formula on oracle/torch_port.mm3;
  * the gate of tests/test_gpu_attn_stream_split_bwd.py catches seven wrong kernels;
  * the new C entries are declared, bound and exported; their workspace queries are host arithmetic with the sizes the header states;
    their refusals happen before anything touches a device; the profiler tags match the header;
  * the Python arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import attn_stream_split_bwd_cases as cases
import attn_stream_split_bwd_ref as ref
from attn_stream_bwd_ref import keep_mask
from oracle import torch_port
from test_gpu_attn_stream_split import worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sumk_attn_stream_split_train", "sumk_attn_stream_split_backward_workspace_bytes", "sumk_attn_stream_split_backward",
       "sumk_transformer_stream_split_train_workspace_bytes", "sumk_transformer_forward_stream_split_train",
       "sumk_transformer_backward_stream_split")
X3 = 1


def _off(lens):
    return (C.c_int32 * (len(lens) + 1))(0, *np.cumsum(lens).tolist())


@pytest.fixture(scope="module")
def lib():
    from summarizer_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", sorted(cases.families()))
def test_x3_yardstick_within_bound_and_spec_passes(name):
    fam = cases.families()[name]
    y3, y32 = cases.yardsticks(fam), cases.yardsticks(fam, which=1)
    print(f"{name}: " + ", ".join(f"{t} x3 {y3[t]:.3e} fp32 {y32[t]:.3e} ratio {y3[t] / y32[t]:.1f}" for t in cases.TENSORS))
    for t in cases.TENSORS:
        assert 0 < y3[t] <= cases.BF16X3_MULT * y32[t], (name, t, y3[t], y32[t])
    for c in fam:                                            # the specification itself is inside the gate, by construction at most 1
        s64, _, s3 = cases.spec(c)
        for t in cases.TENSORS:
            assert np.isfinite(s3[t]).all(), (c["name"], t)
            assert worst(s3[t], s64[t], y3[t], (c["name"], t)) <= 1.0


def _dense_mm3(c):
    """The dense formula with oracle/torch_port.mm3 for all six products, float64 operands, float32 where the accumulators are read."""
    f32 = torch.float32
    sc = np.float32(cases.fwd.scale_of(c))
    p = c["p"]
    ks = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    Q, K, V, G = (torch.from_numpy(c[n]).double() for n in ("q", "k", "v", "dctx"))
    D, heads = c["D"], c["heads"]
    dh = D // heads
    out = {t: torch.zeros(Q.shape[0], D, dtype=torch.float64) for t in cases.TENSORS}
    r0 = 0
    for T in c["lens"]:
        for h in range(heads):
            rows, cols = slice(r0, r0 + T), slice(h * dh, (h + 1) * dh)
            q, k, v, g = (a[rows, cols] for a in (Q, K, V, G))
            keep = torch.from_numpy(keep_mask(cases.SEED, cases.SITE, p, r0, T, heads, h))
            zero = torch.zeros((), dtype=f32)
            e = torch_port.mm3(q, k.t()).to(f32) * sc
            m = e.max(dim=1, keepdim=True).values
            pe = torch.exp(e - m)
            tot = pe.sum(dim=1, keepdim=True)
            pd = torch.where(keep, pe * ks, zero)
            ctx = torch_port.mm3(pd.double(), v).to(f32) / tot
            delta = (g.to(f32) * ctx).sum(dim=1, keepdim=True)
            alpha = pe * (1.0 / tot)
            at = torch.where(keep, alpha * ks, zero)
            dA = torch.where(keep, torch_port.mm3(g, v.t()).to(f32) * ks, zero)
            dS = alpha * (dA - delta) * sc
            out["ctx"][rows, cols] = ctx.double()
            out["dq"][rows, cols] = torch_port.mm3(dS.double(), k).to(f32).double()
            out["dk"][rows, cols] = torch_port.mm3(dS.t().double(), q).to(f32).double()
            out["dv"][rows, cols] = torch_port.mm3(at.t().double(), g).to(f32).double()
        r0 += T
    return {t: a.numpy() for t, a in out.items()}


@pytest.mark.parametrize("D,heads,T,p", ((32, 4, 65, 0.0), (80, 2, 129, 0.5), (256, 2, 200, 0.1)))
def test_float64_accumulation_is_mm3(D, heads, T, p):
    """mha3_train with float64 accumulators = the dense formula on torch_port.mm3: the same planes, the same three plane products in all six
    matrix products, lo.lo dropped.  What is left between them is float32 rounding in two libraries.  For ctx: as in
    test_attn_stream_split_host.test_float64_accumulation_is_mm3, 64 ulps of the largest element (a logit that the two float64 summation
    orders round to neighbouring floats moves a weight by |e| <= 64 ulps).  For the gradients: alpha carries those 64 ulps; dA - delta
    carries one rounding of dA and the difference of two summation orders of delta (dh / 2 ulps of sum |dctx ctx| at most, a few ulps
    typically), taken relative to the LARGEST |dA - delta|; dS is their product, about 64 + 64 ulps of its largest element, and a row of dQ,
    dK or dV is a sum of such terms against the largest element of the result, which the sum's own cancellation can magnify by a small
    factor: 4 x 128 = 512 ulps = 2^-15 bounds them.  A dropped plane product or a one-plane dS or a~ is 2^-9: far outside."""
    c = cases.with_grad(cases.fwd.case(f"mm3b_T{T}_D{D}", (T,), D, heads, 17 + T), p)
    got = ref.mha3_train(c["q"], c["k"], c["v"], c["dctx"], c["lens"], heads, cases.fwd.scale_of(c), p, cases.SEED, cases.SITE, acc=np.float64)
    want = _dense_mm3(c)
    tol = {"ctx": 64 * 2.0 ** -24, "dq": 2.0 ** -15, "dk": 2.0 ** -15, "dv": 2.0 ** -15}
    rel = {t: np.abs(got[t] - want[t]).max() / np.abs(want[t]).max() for t in cases.TENSORS}
    print(f"T{T} D{D} p{p}: " + ", ".join(f"{t} {rel[t] / 2.0 ** -24:.1f} ulps" for t in cases.TENSORS) + " of the largest element")
    for t in cases.TENSORS:
        assert rel[t] <= tol[t], (t, rel[t])
    for mutant, t in (("da_no_lohi", "dq"), ("ds_one_plane", "dq"), ("ds_one_plane", "dk"), ("at_one_plane", "dv")):
        m = ref.mha3_train(c["q"], c["k"], c["v"], c["dctx"], c["lens"], heads, cases.fwd.scale_of(c), p, cases.SEED, cases.SITE, acc=np.float64,
                           mutant=mutant)
        assert np.abs(m[t] - want[t]).max() / np.abs(want[t]).max() > 4 * tol[t], (mutant, t)


# where each mutant is looked for first: the masks need dropout, the neighbouring head a second head
SEARCH = [(256, 2, 0.5), (80, 2, 0.5), (256, 2, 0.1), (80, 2, 0.1)] + [(D, h, 0.0) for D, h in cases.STRIP_SHAPES]


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_gate_catches(mutant):
    """Each wrong kernel fails the GPU test's own worst() in at least one strips family (the search stops at the first case that fails)."""
    for D, heads, p in SEARCH:
        fam = cases.strips(D, heads, p)
        yard = cases.yardsticks(fam)
        for c in reversed(fam):                              # long videos first: more tiles, partial last tiles
            m = ref.mha3_train(c["q"], c["k"], c["v"], c["dctx"], c["lens"], heads, cases.fwd.scale_of(c), p, cases.SEED, cases.SITE, mutant=mutant)
            try:
                for t in cases.TENSORS:
                    worst(m[t], cases.spec(c)[0][t], yard[t], (c["name"], t))
            except AssertionError as e:
                print(f"{mutant}: caught at {c['name']}: {e.args[0]}")
                return
    pytest.fail(f"the gate lets the mutant {mutant} through every strips family")


def test_new_symbols_and_tags(lib):
    from summarizer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sumk.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib._SIGS, name
        assert getattr(lib, name) is not None, name
    tags = {k: int(v) for k, v in re.findall(r"#define (SUMK_PROF_[A-Z0-9_]+) (\d+)", hdr)}
    for i, tag in enumerate(("ATTN_STREAM_SPLIT_BWD_PLANES", "ATTN_STREAM_SPLIT_TRAIN", "ATTN_STREAM_SPLIT_BWD_DQ", "ATTN_STREAM_SPLIT_BWD_DKV")):
        assert tags["SUMK_PROF_" + tag] == getattr(_lib, "PROF_" + tag) == 28 + i, tag
    assert tags["SUMK_PROF_NTAGS"] == _lib.PROF_NTAGS == 32


def test_workspace_queries(lib):
    def bwd(D, heads, lens, prec=X3):
        return int(lib.sumk_attn_stream_split_backward_workspace_bytes(D, heads, len(lens), _off(lens), prec))

    up = lambda b: (b + 255) // 256 * 256
    # descriptors (24 bytes per video) + delta (4 bytes per (row, head)) + seven plane blocks of heads x padded rows x staged columns x 4 bytes
    assert bwd(1024, 8, [64]) == 256 + 64 * 8 * 4 + 7 * 8 * 64 * 128 * 4
    assert bwd(1024, 8, [1]) == 256 + 256 + 7 * 8 * 64 * 128 * 4                                            # videos padded to 64-row tiles
    assert bwd(1024, 8, [65, 1, 64]) == 256 + up(130 * 8 * 4) + 7 * 8 * 256 * 128 * 4                        # ... each on its own
    assert bwd(80, 2, [64]) == 256 + 512 + 7 * 2 * 64 * 64 * 4 and bwd(208, 2, [64]) == 256 + 512 + 7 * 2 * 64 * 128 * 4   # dh 40 -> 64, 104 -> 128
    assert bwd(32, 4, [64]) == 256 + 1024 + 7 * 4 * 64 * 32 * 4
    assert bwd(1024, 8, [64] * 20) == up(24 * 20) + 64 * 20 * 8 * 4 + 7 * 8 * 64 * 20 * 128 * 4
    assert bwd(1024, 8, [65536]) == 256 + 65536 * 8 * 4 + 7 * 65536 * 1024 * 4                               # 28 bytes per element
    for bad in ((8, 2, [10]), (72, 2, [10]), (512, 2, [10]), (64, 3, [10]), (64, 2, [10, 0]), (64, 2, [1 << 20]), (64, 2, [])):
        assert bwd(*bad) == 0, bad
    for prec in (0, 2, 3, 7, -1):
        assert bwd(64, 2, [10], prec) == 0 and f"precision={prec}".encode() in lib.sumk_last_error(), prec
    assert bwd(8, 2, [10]) == 0 and b"head width 4" in lib.sumk_last_error()
    assert bwd(512, 2, [10]) == 0 and b"head width 256" in lib.sumk_last_error()
    # the transformer carve: the stream training carve + the backward's descriptors, delta and planes of ONE layer, whatever the layers
    def tf(D, heads, lens, layers, prec=X3, split=True):
        if split:
            return int(lib.sumk_transformer_stream_split_train_workspace_bytes(D, D, heads, layers, len(lens), _off(lens), prec))
        return int(lib.sumk_transformer_stream_train_workspace_bytes(D, D, heads, layers, len(lens), _off(lens)))
    for lens in ([200, 65], [8192]):
        for layers in (1, 6):
            assert tf(1024, 8, lens, layers) == tf(1024, 8, lens, layers, split=False) + bwd(1024, 8, lens) > 0
    for prec in (0, 2, 3, 7, -1):
        assert tf(64, 2, [10], 2, prec) == 0 and f"precision={prec}".encode() in lib.sumk_last_error(), prec
    assert tf(2048, 8, [10], 2) == 0 and b"head width 256" in lib.sumk_last_error()
    assert tf(72, 2, [10], 2) == 0 and b"head width 36" in lib.sumk_last_error()
    assert tf(64, 2, [10], 0) == 0


def _bwd(lib, D=64, heads=2, lens=(10,), ld=None, p=0.0, ptr=0x10000, dq=None, nb=1 << 24, prec=X3):
    ld = D if ld is None else ld
    return lib.sumk_attn_stream_split_backward(ptr, ld, ptr, ld, ptr, ld, ptr, ld, ptr, ld, ptr, D, heads, len(lens), _off(list(lens)), ptr, 0.125,
                                               p, 1, 0, ptr if dq is None else dq, ld, ptr, ld, ptr, ld, ptr, nb, None, prec)


def _fwd(lib, D=64, heads=2, lens=(10,), ld=None, p=0.0, ptr=0x10000, dq=None, nb=1 << 24, prec=X3):
    ld = D if ld is None else ld
    return lib.sumk_attn_stream_split_train(ptr if dq is None else dq, ld, ptr, ld, ptr, ld, D, heads, len(lens), _off(list(lens)), ptr, 0.125, p, 1,
                                            0, ptr, ld, ptr, ptr, nb, None, prec)


def test_refusals_happen_before_any_device_work(lib):
    """Every call below carries pointers that no device owns: a refusal that came after a launch or a copy would fault, not return."""
    for call in (_bwd, _fwd):
        for prec in (0, 2, 3, 7, -1):
            assert call(lib, prec=prec) == -1 and f"precision={prec}".encode() in lib.sumk_last_error(), prec
        assert call(lib, D=8) == -1 and b"head width 4" in lib.sumk_last_error()
        assert call(lib, D=72) == -1 and b"head width 36" in lib.sumk_last_error()
        assert call(lib, D=512) == -1 and b"head width 256" in lib.sumk_last_error()
        assert call(lib, lens=(0,)) == -1 and b"video 0 has 0 frames" in lib.sumk_last_error()
        assert call(lib, lens=(1 << 20,)) == -1 and b"limit 2^20" in lib.sumk_last_error()
        for p in (-0.1, 1.0, 1.5, float("nan")):
            assert call(lib, p=p) == -1 and b"must lie in [0, 1)" in lib.sumk_last_error(), p
        assert call(lib, ld=60) == -1 and b"must be at least D=64" in lib.sumk_last_error()
        assert call(lib, ld=66) == -1 and b"multiple" in lib.sumk_last_error()
        assert call(lib, nb=16) == -2 and b"workspace 16 < required" in lib.sumk_last_error()
        assert call(lib, dq=0x10004) == -1 and b"16-byte aligned" in lib.sumk_last_error()


def test_python_arguments_without_a_gpu():
    from summarizer_amd import kernels
    from summarizer_amd._lib import SumkError
    sb = kernels.SeqBatch.get([200, 65], torch.device("cpu"))
    a = kernels.attn_stream_backward_workspace_bytes(1024, 8, sb)
    assert a == kernels.attn_stream_backward_workspace_bytes(1024, 8, sb, precision="fp32") == 256 + 265 * 8 * 4 + (256 - 265 * 32 % 256)
    assert kernels.attn_stream_backward_workspace_bytes(1024, 8, sb, precision="bf16x3") == a + 7 * (256 + 128) * 1024 * 4
    x = torch.zeros(265, 64)
    for bad in ("bf16x6", "bf16", "fp16"):
        with pytest.raises(SumkError):
            kernels.attn_stream_backward_workspace_bytes(1024, 8, sb, precision=bad)
        with pytest.raises(SumkError):
            kernels.attn_stream_train(x, x, x, sb, 2, precision=bad)
        with pytest.raises(SumkError):
            kernels.attn_stream_backward(x, x, x, x, x, torch.zeros(265, 2, 2), sb, 2, precision=bad)
    with pytest.raises(SumkError):                           # no CPU path
        kernels.attn_stream_train(x, x, x, sb, 2, precision="bf16x3")
    # what the Transformer scorer's existing tests pin: bf16x3 SCORING does not change training
    with pytest.raises(SumkError):
        kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", training=True, attention_precision="bf16x3")
    t = kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", training=True)
    assert t == kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", training=True, attention_train_precision="fp32")
    assert kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", training=True, attention_train_precision="bf16x3") == \
        t + kernels.attn_stream_backward_workspace_bytes(1024, 8, sb, precision="bf16x3")
    for bad in ("bf16x6", "bf16", "fp16"):
        with pytest.raises(SumkError):
            kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, "stream", training=True, attention_train_precision=bad)
    for kw in (dict(attention="dense", training=True), dict(attention="stream", training=False)):
        with pytest.raises(SumkError):
            kernels.transformer_workspace_bytes(1024, 1024, 8, 6, sb, attention_train_precision="bf16x3", **kw)


def test_model_and_trainer_take_attention_train_precision():
    from summarizer_amd.models.transformer import Transformer, TransformerTrainer
    with pytest.raises(ValueError, match="attention_train_precision must be one of"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention_train="stream", attention_train_precision="bf16x6")
    with pytest.raises(ValueError, match="needs attention_train='stream'"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention_train="dense", attention_train_precision="bf16x3")
    m = Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention_train="stream", attention_train_precision="bf16x3")
    assert m.attention_train_precision == "bf16x3" and m.attention_precision == "fp32" and m.attention == "dense"
    assert Transformer(input_size=64, encoder_layers=1, attention_heads=2).attention_train_precision == "fp32"
    # a model with attention_precision="bf16x3" (scoring) still trains like the fp32 model: its training choice stays the default
    assert Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention="stream", attention_precision="bf16x3").attention_train_precision == "fp32"

    class _Hps:
        extra_params = {"input_size": "64", "encoder_layers": "1", "attention_heads": "2", "attention_train": "stream",
                        "attention_train_precision": "bf16x3"}
        use_cuda = False
    t = TransformerTrainer.__new__(TransformerTrainer)
    t.hps = _Hps()
    m = t._init_model()
    assert m.attention_train == "stream" and m.attention_train_precision == "bf16x3" and m.precision == "fp32"
    _Hps.extra_params = {"input_size": "64", "encoder_layers": "1", "attention_heads": "2", "attention_train": "stream"}
    assert t._init_model().attention_train_precision == "fp32"
    _Hps.extra_params = {"input_size": "64", "encoder_layers": "1", "attention_heads": "2", "attention_train_precision": "bf16x3"}
    with pytest.raises(ValueError, match="needs attention_train='stream'"):
        t._init_model()
