"""GPU: training the Transformer scorer with attention_train="stream", attention_train_precision="bf16x3"
(sumk_transformer_forward_stream_split_train / sumk_transformer_backward_stream_split: every layer's attention on the bf16x3 training form
of csrc/attn_stream_split.hip and on csrc/attn_stream_split_bwd.hip, projections and everything else exact fp32) against the float64
functional reference oracle/torch_port.transformer_ref, with the conventions of tests/test_gpu_transformer_f64.py and the helpers of
tests/test_gpu_transformer_stream_train.py (imported, not edited): TF32 off, the yardstick is the reference's fp32 run, errors are
norm-relative per parameter and per video of dx, dropout is replayed from recipes.transformer_drop_masks.
  Gradient gate: every error is at most BF16X3_MULT = 4 x 2^8 fp32 yardsticks (floor YARD_FLOOR), the project's limit for a bf16x3 model.
  Forward: the training-mode scores at p = 0 lie within 2e-4 of the fp32 stream model's (the gate of tests/test_gpu_transformer_stream_split.py).
  Seeds: the same seed draws the fp32 stream path's masks (the two paths' gradients lie within 2 gates of each other); a second seed moves a
  gradient more than 10 gates away -- other masks on a tenth of the activations move it by tenths of its norm, a gate is about 1e-3 of it.
  Determinism: two runs are bit-equal.  Default: attention_train_precision="fp32" gives the bits of attention_train="stream".
Also the refusals and two epochs of TransformerTrainer with the fp32 attention tags silent.  The figures are kept in REPORT
($SUMK_REPORT_DIR/transformer_stream_split_train.json when set).
Measured on MI355X (2026-10-21), worst gradient error / fp32 yardstick (1024 is the limit) and |bf16x3 - fp32 stream| in gates (2 is the
limit): D = 256 without dropout 37.4 and 0.037, layer dropout 0.1 37.0 and 0.038, layer dropout 0.5 29.3 and 0.029, D = 1024 with 6 layers and
dropout 7.5 and 0.007, more_residuals 10.4 and 0.011, trainable positional table 11.3 and 0.012; |bf16x3 - fp32| on the p = 0 training-mode
scores at most 1.8e-7 (2e-4 is the limit); trainer losses 0.0966248, 0.0812227 beside the fp32 stream trainer's 0.0966248, 0.0812227."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from test_gpu_transformer_f64 import (BF16X3_MULT, R, YARD_FLOOR, _bits, _cw, _err, _names, _nrel, make_inputs, make_model, ref_run)
from test_gpu_transformer_stream_train import SMALL_LENS, hip_train

pytestmark = pytest.mark.gpu
SCORE_GATE = 2e-4
REPORT = []
X3 = "bf16x3"


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
        with open(os.path.join(d, "transformer_stream_split_train.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def hip_train3(m, x, lens, cw, precision, p_layer=0.0, p_head=0.0, seed=0):
    """hip_train on attention="stream" with cfg["attention_train_precision"]: (scores, {name: grad}, dx per video)."""
    from summarizer_amd import kernels
    from summarizer_amd.autograd import TransformerFunction
    names = _names(m)
    sd = dict(m.named_parameters())
    for q in m.parameters():
        q.grad = None
    xg = x.clone().requires_grad_(True)
    opts = dict(layer_eps=1e-5, final_eps=m.epsilon, more_residuals=m.more_residuals, precision="fp32", layer_dropout_p=p_layer,
                head_dropout_p=p_head, seed=seed)
    cfg = dict(n_layers=m.encoder_layers, n_heads=m.attention_heads, dff=m.input_size, attention="stream", attention_train_precision=precision)
    s = TransformerFunction.apply(xg, kernels.SeqBatch.get(lens, x.device), cfg, opts, None, None, names, *[sd[n] for n in names])
    (s * cw).sum().backward()
    return s.detach().clone(), {n: sd[n].grad.clone() for n in names}, [t.clone() for t in torch.split(xg.grad, lens)]


def check(cid, got, fp32, ref64, ref32):
    """got, fp32: (grads, dx) of the bf16x3 and the fp32 stream path; ref64, ref32: those of the reference.  Returns nothing; asserts the gate."""
    worst = beside = 0.0
    items = [(k, got[0][k], fp32[0][k], ref64[0][k], ref32[0][k]) for k in ref64[0]]
    items += [(f"dx{i}", a, d, r, y) for i, (a, d, r, y) in enumerate(zip(got[1], fp32[1], ref64[1], ref32[1]))]
    for k, a, d, r, y in items:
        yard = max(_nrel(y, r), YARD_FLOOR)
        err, gap = _nrel(a, r), _nrel(a, d, scale=float(r.double().norm()))
        worst, beside = max(worst, err / yard), max(beside, gap / (BF16X3_MULT * yard))
        assert err <= BF16X3_MULT * yard, (cid, k, err, yard)
        assert gap <= 2 * BF16X3_MULT * yard, (cid, k, "bf16x3 beside fp32 on the same seed", gap, yard)
    REPORT.append(dict(case=cid, worst_err_over_yardstick=worst, worst_vs_fp32_stream_over_gate=beside))
    print(f"transformer stream split train {cid}: worst gradient {worst:.3f} fp32 yardsticks (limit {BF16X3_MULT:.0f}); "
          f"|bf16x3 - fp32 stream| at most {beside:.4f} gates")


def _case(dev, cid, lens, D, heads, layers, pl, ph, model_seed, **kw):
    seed = 0x5EED1234
    x = make_inputs(lens, D, seed=sum(lens)).to(dev)
    cw = _cw(sum(lens), len(lens)).to(dev)
    m = make_model(D, layers, heads, model_seed, **kw).to(dev).train()
    masks = R.transformer_drop_masks(seed, pl, ph, lens, D, D, heads, layers) if pl or ph else None
    _, u64, g64, dx64 = ref_run(m, x, lens, torch.float64, cw, masks=masks)
    s32, _, g32, dx32 = ref_run(m, x, lens, torch.float32, cw, masks=masks)
    s, g, dx = hip_train3(m, x, lens, cw, X3, pl, ph, seed)
    s2, g2, dx2 = hip_train3(m, x, lens, cw, X3, pl, ph, seed)
    assert torch.equal(_bits(s), _bits(s2)) and all(torch.equal(_bits(g[k]), _bits(g2[k])) for k in g), (cid, "two runs differ")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dx, dx2)), (cid, "two runs differ in dx")
    sf, gf, dxf = hip_train(m, x, lens, cw, "stream", pl, ph, seed)
    assert any(not torch.equal(_bits(g[k]), _bits(gf[k])) for k in g), (cid, "the bf16x3 path gave the fp32 path's bits")
    yard = _err(s32, u64)
    assert _err(s, u64) <= BF16X3_MULT * yard, (cid, "scores", _err(s, u64), yard)
    check(cid, (g, dx), (gf, dxf), (g64, dx64), (g32, dx32))
    if pl or ph:      # another seed: other masks, other gradients
        _, g3, _ = hip_train3(m, x, lens, cw, X3, pl, ph, seed + 1)
        k = "transformer_encoder.layers.0.linear1.weight"
        assert _nrel(g3[k], g64[k]) > 10 * BF16X3_MULT * max(_nrel(g32[k], g64[k]), YARD_FLOOR), (cid, "a second seed drew the same masks")
    # p = 0 in training mode: within the scoring gate of the fp32 stream model's training-mode scores
    s0, _, _ = hip_train3(m, x, lens, cw, X3, 0.0, 0.0, seed)
    sf0, _, _ = hip_train(m, x, lens, cw, "stream", 0.0, 0.0, seed)
    gap = float((s0 - sf0).abs().max())
    print(f"transformer stream split train {cid}: |bf16x3 - fp32| on the p = 0 training-mode scores {gap:.2e} (limit {SCORE_GATE:.0e})")
    assert gap <= SCORE_GATE, (cid, gap)
    REPORT[-1]["score_gap_p0"] = gap
    # the default precision is the fp32 stream path, bit for bit
    sd_, gd_, dxd_ = hip_train3(m, x, lens, cw, "fp32", pl, ph, seed)
    assert torch.equal(_bits(sd_), _bits(sf)) and all(torch.equal(_bits(gd_[k]), _bits(gf[k])) for k in gf), (cid, "fp32 changed its bits")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dxd_, dxf)), (cid, "fp32 changed its bits in dx")


def test_small_without_dropout(dev):
    _case(dev, "small_D256_h2_L2_p0", SMALL_LENS, 256, 2, 2, 0.0, 0.0, 7)


@pytest.mark.parametrize("pl,ph", [(0.1, 0.5), (0.5, 0.5)])
def test_small_with_dropout(dev, pl, ph):
    _case(dev, f"small_D256_h2_L2_p{pl}", SMALL_LENS, 256, 2, 2, pl, ph, 7)


def test_reference_size_with_dropout(dev):
    _case(dev, "reference_D1024_h8_L6_p0.1", [300, 150], 1024, 8, 6, 0.1, 0.5, 27)


def test_more_residuals(dev):
    _case(dev, "more_residuals", SMALL_LENS, 256, 2, 2, 0.1, 0.5, 7, more_residuals=True, epsilon=1e-3)


def test_trainable_positional_table_through_forward(dev):
    """Through Transformer.forward in eval mode with grads enabled (TransformerFunction without dropout): the learnable 'simple' table takes row t
    of every batch entry and its gradient is the scatter of dx."""
    D, heads, layers, T, B = 256, 2, 2, 150, 2
    kw = dict(max_length=200, pos_embed="simple")
    ms = make_model(D, layers, heads, 31, attention_train="stream", attention_train_precision=X3, **kw).to(dev).eval()
    mf = make_model(D, layers, heads, 31, attention_train="stream", **kw).to(dev).eval()
    assert ms.attention_train_precision == X3 and mf.attention_train_precision == "fp32" and ms.attention_precision == "fp32"
    lens = [T] * B
    xp = make_inputs(lens, D, seed=3).to(dev)
    x = xp.view(B, T, D).permute(1, 0, 2).contiguous()
    cw = _cw(B * T, B).to(dev)
    rows = np.arange(B * T) % T
    key = "pos_embed.weight"
    _, u64, g64, dx64 = ref_run(ms, xp, lens, torch.float64, cw, pos=(ms.pos_embed.weight, rows), table_key=key)
    s32, _, g32, dx32 = ref_run(ms, xp, lens, torch.float32, cw, pos=(ms.pos_embed.weight, rows), table_key=key)

    def run(m):
        for q in m.parameters():
            q.grad = None
        xg = x.clone().requires_grad_(True)
        sp = m(xg)[:, :, 0].t().reshape(-1)
        (sp * cw).sum().backward()
        g = {k: q.grad.clone() for k, q in m.named_parameters() if k in g64}
        return sp.detach().clone(), g, [t.clone() for t in torch.split(xg.grad.permute(1, 0, 2).reshape(B * T, D), lens)]
    s, g, dx = run(ms)
    _, gf, dxf = run(mf)
    assert set(g) == set(g64) and key in g
    assert not torch.equal(_bits(g[key]), _bits(gf[key]))
    assert _err(s, u64) <= BF16X3_MULT * _err(s32, u64)
    check("positions_forward", (g, dx), (gf, dxf), (g64, dx64), (g32, dx32))


def test_refusals(dev):
    from summarizer_amd import _lib, kernels
    from summarizer_amd.models.transformer import Transformer
    with pytest.raises(ValueError, match="attention_train_precision must be one of"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention_train="stream", attention_train_precision="bf16x6")
    with pytest.raises(ValueError, match="needs attention_train='stream'"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention_train="dense", attention_train_precision=X3)
    with pytest.raises(ValueError, match="needs attention_train='stream'"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention="stream", attention_precision=X3, attention_train_precision=X3)
    m = make_model(256, 2, 2, 9, attention_train="stream", attention_train_precision=X3).to(dev).train()
    x = make_inputs([70], 256, seed=4).to(dev)
    m.precision = "bf16x3"                                    # a model precision other than fp32 still raises on the stream training path
    with pytest.raises(ValueError, match="attention_train='dense'.*attention_train='stream'"):
        m.score_packed(x, [70])
    torch.manual_seed(0)
    wide = Transformer(input_size=2048, encoder_layers=1, attention_heads=8, attention_train="stream", attention_train_precision=X3).to(dev).train()
    with pytest.raises(_lib.SumkError, match="head width 256"):
        wide.score_packed(torch.zeros(40, 2048, device=dev), [40])
    odd = Transformer(input_size=72, encoder_layers=1, attention_heads=2, attention_train="stream", attention_train_precision=X3).to(dev).train()
    with pytest.raises(_lib.SumkError, match="head width 36"):
        odd.score_packed(torch.zeros(10, 72, device=dev), [10])
    sb = kernels.SeqBatch.get([70], dev)
    with pytest.raises(_lib.SumkError):                       # what the scoring tests pin: attention_precision is not a training argument
        kernels.transformer_workspace_bytes(256, 256, 2, 2, sb, "stream", training=True, attention_precision=X3)
    for bad in (dict(attention="dense", training=True), dict(attention="stream", training=False)):
        with pytest.raises(_lib.SumkError):
            kernels.transformer_workspace_bytes(256, 256, 2, 2, sb, attention_train_precision=X3, **bad)
    a = kernels.transformer_workspace_bytes(256, 256, 2, 2, sb, "stream", training=True)
    b = kernels.transformer_workspace_bytes(256, 256, 2, 2, sb, "stream", training=True, attention_train_precision=X3)
    assert b == a + kernels.attn_stream_backward_workspace_bytes(256, 2, sb, precision=X3)


def test_trainer_two_epochs_and_the_fp32_attention_tags_stay_silent(dev):
    from summarizer_amd import _lib
    from summarizer_amd.models.transformer import TransformerTrainer
    from summarizer_amd.utils.datasets import synthetic_dataset
    from summarizer_amd.utils.hps import make_hps
    lib = _lib.load()
    ds = synthetic_dataset(5, seed=3, D=128, t_range=(40, 90), n_users=5)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))

    def losses(extra):
        hps = make_hps(ds, [{"train_keys": keys[1:], "test_keys": keys[:1]}], epochs=2, test_every_epochs=1, lr=3e-4, selection_algorithm="rank",
                       extra_params=dict({"input_size": "128", "encoder_layers": "2", "attention_heads": "4", "batch_videos": "2",
                                          "attention": "stream", "attention_train": "stream"}, **extra))
        torch.manual_seed(4); random.seed(4)
        tr = TransformerTrainer(hps, hps.splits_files[0]).reset()
        tr.train(0)
        return tr, [v for _, v in hps.writer.scalars["synthetic/Fold_1/Train/Loss"]]
    _, fp32 = losses({})
    ms, n = C.c_double(0), C.c_int64(0)
    silent = (_lib.PROF_TF_ATTN_DENSE, _lib.PROF_ATTN_STREAM_TRAIN, _lib.PROF_ATTN_STREAM_BWD_DQ, _lib.PROF_ATTN_STREAM_BWD_DKV)
    loud = (_lib.PROF_ATTN_STREAM_SPLIT_TRAIN, _lib.PROF_ATTN_STREAM_SPLIT_BWD_PLANES, _lib.PROF_ATTN_STREAM_SPLIT_BWD_DQ,
            _lib.PROF_ATTN_STREAM_SPLIT_BWD_DKV, _lib.PROF_ATTN_STREAM_BWD_DELTA)
    for t in silent + loud:
        lib.sumk_prof_read(t, None, None, 1)
    lib.sumk_prof_enable(sum(1 << t for t in silent + loud))
    try:
        tr, x3 = losses({"attention_train_precision": X3})
        torch.cuda.synchronize()
        counts = {}
        for t in silent + loud:
            lib.sumk_prof_read(t, C.byref(ms), C.byref(n), 1)
            counts[t] = n.value
    finally:
        lib.sumk_prof_enable(0)
    assert tr.model.attention_train == "stream" and tr.model.attention_train_precision == X3
    steps = 2 * 2 * 2                                         # epochs x steps per epoch x layers
    assert all(counts[t] == 0 for t in silent), counts
    assert all(counts[t] == steps for t in loud), counts
    print(f"transformer stream split train trainer: losses bf16x3 {x3} beside fp32 stream {fp32}")
    assert len(fp32) == len(x3) == 2 and np.isfinite(fp32).all() and np.isfinite(x3).all()
    REPORT.append(dict(case="trainer", fp32_stream_losses=fp32, bf16x3_losses=x3))
