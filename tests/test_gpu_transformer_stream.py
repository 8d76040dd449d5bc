"""GPU: the Transformer scorer with attention="stream" (sumk_transformer_forward_stream: every layer's attention on csrc/attn_stream.hip, no
(T x T) logits in the workspace) against the float64 functional reference oracle/torch_port.transformer_ref, with the inputs, the model
recipe and the gate of tests/test_gpu_transformer_f64.py: the yardstick is the same reference run in fp32, the gate 4 yardsticks on the
logits recovered from the scores (k2 scaled by K2_SCALE so that the scores stay inside (0.01, 0.99)).  Beside the dense model on the same
weights the two paths must lie within 2 gates of each other.  Also: more_residuals and a positional table through forward(), the autograd
branch (dense path, gradients bit-equal to attention="dense"), the refusal of other precisions, and a Summarizer run.
The figures are kept in REPORT (written to $SUMK_REPORT_DIR/transformer_stream.json when set).
Measured on MI355X (2026-10-20), error / yardstick (4 is the limit): D = 256 1.06, D = 1024 with 6 layers 0.80, more_residuals 0.99, positional
table 0.76; |stream - dense| on the logits at most 7.2e-7."""
import json
import os

import numpy as np
import pytest
import torch

import kts_ref
from test_gpu_transformer_f64 import FP32_MULT, _err, _logit, make_inputs, make_model, ref_run

pytestmark = pytest.mark.gpu
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
        with open(os.path.join(d, "transformer_stream.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def _pair(dev, D, layers, heads, seed, **kw):
    """The same weights behind attention="stream" and attention="dense"."""
    s = make_model(D, layers, heads, seed, attention="stream", **kw).to(dev).eval()
    d = make_model(D, layers, heads, seed, **kw).to(dev).eval()
    assert s.attention == "stream" and d.attention == "dense"
    return s, d


def _case(dev, cid, lens, D, heads, layers, **kw):
    x = make_inputs(lens, D, seed=sum(lens) + heads).to(dev)
    ms, md = _pair(dev, D, layers, heads, 5 + layers, **kw)
    with torch.no_grad():
        s64, u64 = ref_run(ms, x, lens, torch.float64)
        s32, _ = ref_run(ms, x, lens, torch.float32)
        a = ms.score_packed(x, lens).clone()
        b = ms.score_packed(x, lens).clone()
        dn = md.score_packed(x, lens).clone()
    assert float(s64.min()) > 0.01 and float(s64.max()) < 0.99
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (cid, "two calls differ")
    yard = _err(s32, u64)
    err, gate = _err(a, u64), FP32_MULT * yard
    beside = float((_logit(a) - _logit(dn)).abs().max())
    REPORT.append(dict(case=cid, err=err, yardstick=yard, gate=gate, err_over_yardstick=err / yard, dense_err=_err(dn, u64), stream_vs_dense=beside))
    print(f"transformer stream {cid}: {err / yard:.3f} yardsticks ({yard:.3e}); dense {_err(dn, u64) / yard:.3f}; |stream - dense| {beside:.3e}")
    assert err <= gate, (cid, err, yard, gate)
    assert beside <= 2 * gate, (cid, beside, gate)


def test_model_small(dev):
    _case(dev, "small_D256_h2_L2", [1, 63, 64, 65, 129, 200, 321], 256, 2, 2)


def test_model_reference_size(dev):
    _case(dev, "reference_D1024_h8_L6", [300, 150], 1024, 8, 6)


def test_more_residuals(dev):
    _case(dev, "more_residuals", [1, 63, 64, 65, 129, 200, 321], 256, 2, 2, more_residuals=True, epsilon=1e-3)


def test_positional_table_through_forward(dev):
    D, heads, layers, T, B = 256, 2, 2, 150, 2
    ms, md = _pair(dev, D, layers, heads, 31, max_length=200, pos_embed="simple")
    lens = [T] * B
    xp = make_inputs(lens, D, seed=3).to(dev)
    x = xp.view(B, T, D).permute(1, 0, 2).contiguous()
    rows = np.arange(B * T) % T
    with torch.no_grad():
        _, u64 = ref_run(ms, xp, lens, torch.float64, pos=(ms.pos_embed.weight, rows))
        s32, _ = ref_run(ms, xp, lens, torch.float32, pos=(ms.pos_embed.weight, rows))
        a = ms(x.clone())[:, :, 0].t().reshape(-1)
        dn = md(x.clone())[:, :, 0].t().reshape(-1)
        sp = ms.score_packed(xp, lens)                      # the packed route adds the positions out of place
    yard = _err(s32, u64)
    err, gate = _err(a, u64), FP32_MULT * yard
    REPORT.append(dict(case="positions_forward", err=err, yardstick=yard, gate=gate, err_over_yardstick=err / yard))
    print(f"transformer stream positions: {err / yard:.3f} yardsticks ({yard:.3e})")
    assert err <= gate and _err(sp, u64) <= gate
    assert float((_logit(a) - _logit(dn)).abs().max()) <= 2 * gate


def test_autograd_stays_dense_and_bit_equal(dev):
    lens, D = [65, 130], 256
    ms, md = _pair(dev, D, 2, 2, 9)
    x = make_inputs(lens, D, seed=4).to(dev)
    cw = torch.from_numpy(np.random.default_rng(1).standard_normal(sum(lens)).astype(np.float32)).to(dev)
    grads = []
    for m in (ms, md):
        for q in m.parameters():
            q.grad = None
        s = m.score_packed(x, lens)                         # grads enabled, eval mode: TransformerFunction without dropout
        assert s.requires_grad
        (s * cw).sum().backward()
        grads.append({k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    for k in grads[0]:
        assert torch.equal(grads[0][k].view(torch.int32), grads[1][k].view(torch.int32)), k


def test_other_precisions_raise(dev):
    ms, _ = _pair(dev, 256, 2, 2, 9)
    x = make_inputs([70], 256, seed=4).to(dev)
    ms.precision = "bf16x6"
    with torch.no_grad(), pytest.raises(ValueError, match="attention='dense'.*attention='stream'"):
        ms.score_packed(x, [70])
    from summarizer_amd.models.transformer import Transformer
    with pytest.raises(ValueError, match="dense.*stream"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention="flash")


def test_summarizer_with_a_stream_model(dev):
    import summarizer_amd
    n, D = 700, 256
    ms, md = _pair(dev, D, 2, 2, 13)
    X = kts_ref.planted_features(n, D, 12, 0.05, 700)[0]
    feats = [torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)]
    kw = dict(kts="banded", device=True, tail="long")
    got = summarizer_amd.Summarizer(ms, **kw).summarize_batch(feats)[0]
    want = summarizer_amd.Summarizer(md, **kw).summarize_batch(feats)[0]
    torch.cuda.synchronize()
    assert int(got["status"]) == 0 and int(want["status"]) == 0
    assert int(got["n_segs"]) == int(want["n_segs"]) > 1
    assert torch.equal(got["change_points"], want["change_points"])
    assert torch.equal(got["machine_summary"], want["machine_summary"]) and 0 < float(got["machine_summary"].sum()) <= 0.15 * n + 1
    REPORT.append(dict(case="summarizer_n700", n_segs=int(got["n_segs"]), summary_frames=int(got["machine_summary"].sum()),
                       stream_vs_dense_scores=float((got["scores"] - want["scores"]).abs().max())))
