"""GPU: the Transformer scorer with attention="stream", attention_precision="bf16x3" (sumk_transformer_forward_stream_split: every layer's
attention on csrc/attn_stream_split.hip, the projections exact fp32) against the float64 functional reference
oracle/torch_port.transformer_ref, with the inputs and the model recipe of tests/test_gpu_transformer_f64.py (k2 scaled by K2_SCALE so that
the scores stay inside (0.01, 0.99), logits recovered from the scores).
  Gate 1: the logits lie within BF16X3_MULT = 4 x 2^8 fp32 yardsticks of the float64 reference (the yardstick: the same reference in fp32).
  Gate 2: the scores lie within 2e-4 of the fp32 stream model's on the same weights (the gate tests/test_gpu_fuzz_planes.py holds bf16x3
          scoring to).
Also: more_residuals and a positional table through forward(), the autograd branch (bit-equal to attention_precision="fp32"), the
constructor's refusals, and a Summarizer run.  The figures are kept in REPORT ($SUMK_REPORT_DIR/transformer_stream_split.json when set).
Measured on MI355X (2026-10-21), gate 1, error / fp32 yardstick (1024 is the limit): D = 256 1.65, D = 1024 with 6 layers 0.75, more_residuals
1.14, positional table 1.09; gate 2, |bf16x3 - fp32| on the scores: at most 2.1e-7 (2e-4 is the limit)."""
import json
import os

import numpy as np
import pytest
import torch

import kts_ref
from test_gpu_transformer_f64 import BF16X3_MULT, _err, _logit, make_inputs, make_model, ref_run

pytestmark = pytest.mark.gpu
SCORE_GATE = 2e-4
REPORT = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    prev = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32, torch.get_float32_matmul_precision())
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    yield torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = prev[:2]
    torch.set_float32_matmul_precision(prev[2])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "transformer_stream_split.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def _pair(dev, D, layers, heads, seed, **kw):
    """The same weights behind the bf16x3 and the fp32 attention of the stream path."""
    s = make_model(D, layers, heads, seed, attention="stream", attention_precision="bf16x3", **kw).to(dev).eval()
    f = make_model(D, layers, heads, seed, attention="stream", **kw).to(dev).eval()
    assert s.attention_precision == "bf16x3" and f.attention_precision == "fp32" and s.attention == f.attention == "stream"
    return s, f


def _gates(cid, a, f, s32, u64):
    yard = _err(s32, u64)
    err, gate = _err(a, u64), BF16X3_MULT * yard
    beside = float((a - f).abs().max())
    REPORT.append(dict(case=cid, err=err, yardstick=yard, gate=gate, err_over_yardstick=err / yard, fp32_stream_err_over_yardstick=_err(f, u64) / yard,
                       split_vs_fp32_scores=beside, score_gate=SCORE_GATE))
    print(f"transformer stream split {cid}: {err / yard:.3f} yardsticks ({yard:.3e}; limit {BF16X3_MULT:.0f}); fp32 stream {_err(f, u64) / yard:.3f}; "
          f"|split - fp32| on the scores {beside:.3e} (limit {SCORE_GATE:.0e})")
    assert err <= gate, (cid, err, yard, gate)
    assert beside <= SCORE_GATE, (cid, beside)
    assert not torch.equal(a.view(torch.int32), f.view(torch.int32)), (cid, "the bf16x3 model gave the fp32 model's bits")


def _case(dev, cid, lens, D, heads, layers, **kw):
    x = make_inputs(lens, D, seed=sum(lens) + heads).to(dev)
    ms, mf = _pair(dev, D, layers, heads, 5 + layers, **kw)
    with torch.no_grad():
        s64, u64 = ref_run(ms, x, lens, torch.float64)
        s32, _ = ref_run(ms, x, lens, torch.float32)
        a = ms.score_packed(x, lens).clone()
        b = ms.score_packed(x, lens).clone()
        f = mf.score_packed(x, lens).clone()
    assert float(s64.min()) > 0.01 and float(s64.max()) < 0.99
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (cid, "two calls differ")
    _gates(cid, a, f, s32, u64)


def test_model_small(dev):
    _case(dev, "small_D256_h2_L2", [70, 130, 257], 256, 2, 2)


def test_model_reference_size(dev):
    _case(dev, "reference_D1024_h8_L6", [200, 65], 1024, 8, 6)


def test_more_residuals(dev):
    _case(dev, "more_residuals", [70, 130, 257], 256, 2, 2, more_residuals=True, epsilon=1e-3)


def test_positional_table_through_forward(dev):
    D, heads, layers, T, B = 256, 2, 2, 150, 2
    ms, mf = _pair(dev, D, layers, heads, 31, max_length=200, pos_embed="simple")
    lens = [T] * B
    xp = make_inputs(lens, D, seed=3).to(dev)
    x = xp.view(B, T, D).permute(1, 0, 2).contiguous()
    rows = np.arange(B * T) % T
    with torch.no_grad():
        _, u64 = ref_run(ms, xp, lens, torch.float64, pos=(ms.pos_embed.weight, rows))
        s32, _ = ref_run(ms, xp, lens, torch.float32, pos=(ms.pos_embed.weight, rows))
        a = ms(x.clone())[:, :, 0].t().reshape(-1)
        f = mf(x.clone())[:, :, 0].t().reshape(-1)
        sp = ms.score_packed(xp, lens)                      # the packed route adds the positions out of place
    _gates("positions_forward", a, f, s32, u64)
    assert _err(sp, u64) <= BF16X3_MULT * _err(s32, u64)


def test_autograd_follows_attention_train_bit_equal(dev):
    """attention_precision governs the no-grad branch alone: under autograd the bf16x3 model gives the fp32 model's scores and gradients,
    bit for bit, on both attention_train paths."""
    lens, D = [65, 130], 256
    x = make_inputs(lens, D, seed=4).to(dev)
    cw = torch.from_numpy(np.random.default_rng(1).standard_normal(sum(lens)).astype(np.float32)).to(dev)
    for train in ("dense", "stream"):
        ms, mf = _pair(dev, D, 2, 2, 9, attention_train=train)
        res = []
        for m in (ms, mf):
            for q in m.parameters():
                q.grad = None
            s = m.score_packed(x, lens)                     # grads enabled, eval mode: TransformerFunction without dropout
            assert s.requires_grad
            (s * cw).sum().backward()
            res.append((s.detach().clone(), {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}))
        assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)), train
        assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 10
        for k in res[0][1]:
            assert torch.equal(res[0][1][k].view(torch.int32), res[1][1][k].view(torch.int32)), (train, k)


def test_refusals(dev):
    from summarizer_amd.models.transformer import Transformer
    with pytest.raises(ValueError, match="attention_precision must be one of"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention="stream", attention_precision="bf16x6")
    with pytest.raises(ValueError, match="needs attention='stream'"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention="dense", attention_precision="bf16x3")
    # the model `precision` refusal of the stream path stands beside the new knob
    ms, _ = _pair(dev, 256, 2, 2, 9)
    ms.precision = "bf16x3"
    with torch.no_grad(), pytest.raises(ValueError, match="attention='dense'.*attention='stream'"):
        ms.score_packed(make_inputs([70], 256, seed=4).to(dev), [70])
    # a head width the bf16x3 kernel refuses is an error, not another path
    from summarizer_amd._lib import SumkError
    m = Transformer(input_size=72, encoder_layers=1, attention_heads=2, attention="stream", attention_precision="bf16x3").to(dev).eval()
    with torch.no_grad(), pytest.raises(SumkError, match="head width 36"):
        m.score_packed(torch.zeros(10, 72, device=dev), [10])


def test_summarizer_with_a_split_model(dev):
    import summarizer_amd
    n, D = 700, 256
    ms, mf = _pair(dev, D, 2, 2, 13)
    X = kts_ref.planted_features(n, D, 12, 0.05, 700)[0]
    feats = [torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)]
    kw = dict(kts="banded", device=True, tail="long")
    got = summarizer_amd.Summarizer(ms, **kw).summarize_batch(feats)[0]
    want = summarizer_amd.Summarizer(mf, **kw).summarize_batch(feats)[0]
    torch.cuda.synchronize()
    assert int(got["status"]) == 0 and int(want["status"]) == 0
    assert int(got["n_segs"]) == int(want["n_segs"]) > 1
    assert torch.equal(got["change_points"], want["change_points"])
    beside = float((got["scores"] - want["scores"]).abs().max())
    assert 0 < beside <= SCORE_GATE, beside
    assert 0 < float(got["machine_summary"].sum()) <= 0.15 * n + 1
    REPORT.append(dict(case="summarizer_n700", n_segs=int(got["n_segs"]), summary_frames=int(got["machine_summary"].sum()),
                       split_vs_fp32_scores=beside, same_summary=bool(torch.equal(got["machine_summary"], want["machine_summary"]))))
