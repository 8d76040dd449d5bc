"""GPU: training the Transformer scorer with attention_train="stream" (sumk_transformer_forward_stream_train / sumk_transformer_backward_stream:
every layer's attention on csrc/attn_stream.hip's training form and csrc/attn_stream_bwd.hip, no (T x T) block in the workspace) against
the float64 functional reference oracle/torch_port.transformer_ref, with the conventions of tests/test_gpu_transformer_f64.py: TF32 off, the
yardstick is the reference's fp32 run, errors are norm-relative per parameter and per video of dx, the gate is 4 yardsticks (floor
YARD_FLOOR), dropout is replayed from recipes.transformer_drop_masks.  Beside the dense path on the same weights and the same seed (hence
the same masks) every gradient must lie within 2 gates; another seed must give other gradients; p = 0 in training mode must give the
eval-mode scores of attention="stream" bit for bit.  Also: more_residuals, a trainable positional table (its gradient comes through dx),
the refusals, and two epochs of TransformerTrainer with the dense attention's profiler tag silent.
The figures are kept in REPORT (written to $SUMK_REPORT_DIR/transformer_stream_train.json when set).
Measured on MI355X (2026-10-20), worst gradient error / yardstick (4 is the limit) and |stream - dense| in gates (2 is the limit): D = 256 without
dropout 1.54 and 0.34, layer dropout 0.1 2.52 and 0.64, layer dropout 0.5 1.79 and 0.42, D = 1024 with 6 layers and dropout 1.35 and 0.36,
more_residuals 1.69 and 0.42, trainable positional table 1.40 and 0.31."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from test_gpu_transformer_f64 import (FP32_MULT, R, YARD_FLOOR, _bits, _cw, _err, _names, _nrel, make_inputs, make_model, ref_run)

pytestmark = pytest.mark.gpu
REPORT = []
SMALL_LENS = [1, 63, 64, 65, 129, 200, 321]


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
        with open(os.path.join(d, "transformer_stream_train.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


def hip_train(m, x, lens, cw, attention, p_layer=0.0, p_head=0.0, seed=0):
    """One forward + backward through TransformerFunction with an explicit dropout seed and attention: (scores, {name: grad}, dx per video)."""
    from summarizer_amd import kernels
    from summarizer_amd.autograd import TransformerFunction
    names = _names(m)
    sd = dict(m.named_parameters())
    for q in m.parameters():
        q.grad = None
    xg = x.clone().requires_grad_(True)
    opts = dict(layer_eps=1e-5, final_eps=m.epsilon, more_residuals=m.more_residuals, precision="fp32", layer_dropout_p=p_layer,
                head_dropout_p=p_head, seed=seed)
    cfg = dict(n_layers=m.encoder_layers, n_heads=m.attention_heads, dff=m.input_size, attention=attention)
    s = TransformerFunction.apply(xg, kernels.SeqBatch.get(lens, x.device), cfg, opts, None, None, names, *[sd[n] for n in names])
    (s * cw).sum().backward()
    return s.detach().clone(), {n: sd[n].grad.clone() for n in names}, [t.clone() for t in torch.split(xg.grad, lens)]


def check(cid, got, dense, ref64, ref32):
    """got, dense: (grads, dx) of the stream and the dense path; ref64, ref32: those of the reference.  Returns the worst error / yardstick."""
    worst = beside = 0.0
    items = [(k, got[0][k], dense[0][k], ref64[0][k], ref32[0][k]) for k in ref64[0]]
    items += [(f"dx{i}", a, d, r, y) for i, (a, d, r, y) in enumerate(zip(got[1], dense[1], ref64[1], ref32[1]))]
    for k, a, d, r, y in items:
        yard = max(_nrel(y, r), YARD_FLOOR)
        err, gap = _nrel(a, r), _nrel(a, d, scale=float(r.double().norm()))
        worst, beside = max(worst, err / yard), max(beside, gap / (FP32_MULT * yard))
        assert err <= FP32_MULT * yard, (cid, k, err, yard)
        assert gap <= 2 * FP32_MULT * yard, (cid, k, "stream beside dense", gap, yard)
    REPORT.append(dict(case=cid, worst_err_over_yardstick=worst, worst_stream_vs_dense_over_gate=beside))
    print(f"transformer stream train {cid}: worst gradient {worst:.3f} yardsticks; |stream - dense| at most {beside:.3f} gates")


def _case(dev, cid, lens, D, heads, layers, pl, ph, model_seed, **kw):
    seed = 0x5EED1234
    x = make_inputs(lens, D, seed=sum(lens)).to(dev)
    cw = _cw(sum(lens), len(lens)).to(dev)
    m = make_model(D, layers, heads, model_seed, **kw).to(dev).train()
    masks = R.transformer_drop_masks(seed, pl, ph, lens, D, D, heads, layers) if pl or ph else None
    _, u64, g64, dx64 = ref_run(m, x, lens, torch.float64, cw, masks=masks)
    s32, _, g32, dx32 = ref_run(m, x, lens, torch.float32, cw, masks=masks)
    s, g, dx = hip_train(m, x, lens, cw, "stream", pl, ph, seed)
    s2, g2, dx2 = hip_train(m, x, lens, cw, "stream", pl, ph, seed)
    assert torch.equal(_bits(s), _bits(s2)) and all(torch.equal(_bits(g[k]), _bits(g2[k])) for k in g), (cid, "two runs differ")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dx, dx2)), (cid, "two runs differ in dx")
    sd, gd, dxd = hip_train(m, x, lens, cw, "dense", pl, ph, seed)
    yard = _err(s32, u64)
    assert _err(s, u64) <= FP32_MULT * yard, (cid, "scores", _err(s, u64), yard)
    check(cid, (g, dx), (gd, dxd), (g64, dx64), (g32, dx32))
    if pl or ph:      # another seed: other masks, other gradients (far outside the gate around this seed's reference)
        _, g3, _ = hip_train(m, x, lens, cw, "stream", pl, ph, seed + 1)
        k = "transformer_encoder.layers.0.linear1.weight"
        assert _nrel(g3[k], g64[k]) > 100 * FP32_MULT * max(_nrel(g32[k], g64[k]), YARD_FLOOR), (cid, "a second seed drew the same masks")
    # p = 0 in training mode: the eval-mode scores of attention="stream", bit for bit
    s0, _, _ = hip_train(m, x, lens, cw, "stream", 0.0, 0.0, seed)
    m.eval()
    m.attention = "stream"
    with torch.no_grad():
        se = m.score_packed(x, lens).clone()
    assert torch.equal(_bits(s0), _bits(se)), (cid, "the p = 0 training forward differs from eval mode")


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
    ms = make_model(D, layers, heads, 31, attention_train="stream", **kw).to(dev).eval()
    md = make_model(D, layers, heads, 31, **kw).to(dev).eval()
    assert ms.attention_train == "stream" and md.attention_train == "dense" and ms.attention == "dense"
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
    _, gd, dxd = run(md)
    assert set(g) == set(g64) and key in g
    assert _err(s, u64) <= FP32_MULT * _err(s32, u64)
    check("positions_forward", (g, dx), (gd, dxd), (g64, dx64), (g32, dx32))


def test_refusals(dev):
    from summarizer_amd import _lib
    from summarizer_amd.models.transformer import Transformer
    m = make_model(256, 2, 2, 9, attention_train="stream").to(dev).train()
    x = make_inputs([70], 256, seed=4).to(dev)
    m.precision = "bf16x3"
    with pytest.raises(ValueError, match="attention_train='dense'.*attention_train='stream'"):
        m.score_packed(x, [70])
    with pytest.raises(ValueError, match="dense.*stream"):
        Transformer(input_size=64, encoder_layers=1, attention_heads=2, attention_train="flash")
    torch.manual_seed(0)
    wide = Transformer(input_size=2048, encoder_layers=1, attention_heads=8, attention_train="stream").to(dev).train()
    with pytest.raises(_lib.SumkError, match="head width 256"):
        wide.score_packed(torch.zeros(40, 2048, device=dev), [40])


def test_trainer_two_epochs_match_dense_and_never_launch_the_dense_core(dev):
    from summarizer_amd import _lib
    from summarizer_amd.models.transformer import TransformerTrainer
    from summarizer_amd.utils.datasets import synthetic_dataset
    from summarizer_amd.utils.hps import make_hps
    lib = _lib.load()
    ds = synthetic_dataset(5, seed=3, D=128, t_range=(40, 90), n_users=5)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))

    def losses(extra):
        hps = make_hps(ds, [{"train_keys": keys[1:], "test_keys": keys[:1]}], epochs=2, test_every_epochs=1, lr=3e-4, selection_algorithm="rank",
                       extra_params=dict({"input_size": "128", "encoder_layers": "2", "attention_heads": "4", "batch_videos": "2"}, **extra))
        torch.manual_seed(4); random.seed(4)
        tr = TransformerTrainer(hps, hps.splits_files[0]).reset()
        tr.train(0)
        return tr, [v for _, v in hps.writer.scalars["synthetic/Fold_1/Train/Loss"]]
    _, dense = losses({})
    ms, n = C.c_double(0), C.c_int64(0)
    tags = (_lib.PROF_TF_ATTN_DENSE, _lib.PROF_ATTN_STREAM_TRAIN, _lib.PROF_ATTN_STREAM_BWD_DQ, _lib.PROF_ATTN_STREAM_BWD_DKV)
    for t in tags:
        lib.sumk_prof_read(t, None, None, 1)
    lib.sumk_prof_enable(sum(1 << t for t in tags))
    try:
        tr, stream = losses({"attention": "stream", "attention_train": "stream"})
        torch.cuda.synchronize()
        counts = {}
        for t in tags:
            lib.sumk_prof_read(t, C.byref(ms), C.byref(n), 1)
            counts[t] = n.value
    finally:
        lib.sumk_prof_enable(0)
    assert tr.model.attention_train == "stream"
    assert counts[_lib.PROF_TF_ATTN_DENSE] == 0, counts
    steps = 2 * 2 * 2                                         # epochs x steps per epoch x layers
    assert counts[_lib.PROF_ATTN_STREAM_TRAIN] == counts[_lib.PROF_ATTN_STREAM_BWD_DQ] == counts[_lib.PROF_ATTN_STREAM_BWD_DKV] == steps, counts
    assert len(dense) == len(stream) == 2 and np.isfinite(dense).all()
    assert np.allclose(stream, dense, rtol=1e-4, atol=0), (stream, dense)
    REPORT.append(dict(case="trainer", dense_losses=dense, stream_losses=stream))
