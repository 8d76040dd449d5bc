"""GPU: the SumGAN-Att stacks (csrc/tf_decoder.hip) -- decoder stack and encoder-stack entry against torch's own modules in float64
on the CPU, forward and backward; determinism and dropout masks; poisoned allocations; packed batches; the model classes of
summarizer_amd.models.sumgan_att against the stock modules they hold."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # forward atol, as tests/test_gpu_transformer.py
GRAD_REL = 3e-4                 # per-tensor relative gradient error, as tests/test_gpu_transformer.py
LENS_FULL = [1, 63, 64, 65, 320, 321, 650]
LENS_SMALL = [1, 17, 40]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _decoder(D, H, L, seed):
    torch.manual_seed(seed)
    layer = nn.TransformerDecoderLayer(d_model=D, nhead=H, dim_feedforward=D, dropout=0.0)
    return nn.TransformerDecoder(layer, num_layers=L)


def _encoder(D, H, L, seed, norm):
    torch.manual_seed(seed)
    layer = nn.TransformerEncoderLayer(d_model=D, nhead=H, dim_feedforward=D, dropout=0.0)
    return nn.TransformerEncoder(layer, num_layers=L, norm=nn.LayerNorm(D) if norm else None, enable_nested_tensor=False)


def _randomise_norms(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn(p.shape, generator=g))


def _ref_fwd_bwd(fn, mod, inputs, lens, G):
    """float64 CPU: per video fn(mod, *pieces) with pieces (T,1,D); loss = sum(out * G).  -> out, input grads, param grads"""
    m = mod.double()
    for p in m.parameters():
        p.grad = None
    xs = [t.detach().double().clone().requires_grad_(True) for t in inputs]
    off = np.concatenate([[0], np.cumsum(lens)])
    outs = [fn(m, *[x[off[i]:off[i + 1]].unsqueeze(1) for x in xs]).squeeze(1) for i in range(len(lens))]
    out = torch.cat(outs)
    (out * G.double()).sum().backward()
    res = (out.detach().numpy(), [x.grad.numpy() for x in xs], {n: p.grad.numpy().copy() for n, p in m.named_parameters()})
    mod.float()
    return res


def _hip_decoder(dec, tgt, mem, lens, G, dev, opts=None, n_heads=4):
    from summarizer_amd import kernels
    from summarizer_amd.autograd import TfDecoderFunction
    L = dec.num_layers
    names = kernels.tf_decoder_param_names("layers.", L)
    p = dict(dec.named_parameters())
    ts = [p[n].detach().float().to(dev).contiguous().requires_grad_(True) for n in names]
    t = tgt.float().to(dev).requires_grad_(True)
    m = mem.float().to(dev).requires_grad_(True)
    sb = kernels.SeqBatch.get(lens, dev)
    cfg = dict(n_layers=L, n_heads=n_heads, dff=dec.layers[0].linear1.out_features)
    out = TfDecoderFunction.apply(t, m, sb, cfg, opts or dict(layer_eps=1e-5), names, *ts)
    out.backward(G.float().to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), [t.grad.cpu().numpy(), m.grad.cpu().numpy()], {n: q.grad.cpu().numpy() for n, q in zip(names, ts)}


def _hip_encoder(enc, x, lens, G, dev, n_heads=4):
    from summarizer_amd import kernels
    from summarizer_amd.autograd import TfEncoderFunction
    L = enc.num_layers
    names = kernels.tf_encoder_param_names("layers.", L, "norm." if enc.norm is not None else None)
    p = dict(enc.named_parameters())
    ts = [p[n].detach().float().to(dev).contiguous().requires_grad_(True) for n in names]
    xd = x.float().to(dev).requires_grad_(True)
    sb = kernels.SeqBatch.get(lens, dev)
    cfg = dict(n_layers=L, n_heads=n_heads, dff=enc.layers[0].linear1.out_features)
    out = TfEncoderFunction.apply(xd, sb, cfg, dict(layer_eps=1e-5, final_eps=1e-5), names, *ts)
    out.backward(G.float().to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), [xd.grad.cpu().numpy()], {n: q.grad.cpu().numpy() for n, q in zip(names, ts)}


def _compare(hip, ref, what):
    y, dins, dps = hip
    y_r, dins_r, dps_r = ref
    np.testing.assert_allclose(y, y_r, atol=TOL, rtol=0, err_msg=f"{what} forward")
    for i, (a, b) in enumerate(zip(dins, dins_r)):
        assert rel(a, b) < GRAD_REL, (what, "input", i, rel(a, b))
    for n, a in dps.items():
        assert rel(a, dps_r[n]) < GRAD_REL, (what, n, rel(a, dps_r[n]))


def _inputs(lens, D, seed, n=2):
    g = torch.Generator().manual_seed(seed)
    R = sum(lens)
    return [torch.randn(R, D, generator=g) for _ in range(n)] + [torch.randn(R, D, generator=g)]


@pytest.mark.parametrize("D,H,L,lens", [(64, 4, 2, LENS_SMALL), (1024, 4, 2, LENS_FULL)], ids=["small", "full"])
def test_decoder_stack_vs_torch_fp64(dev, D, H, L, lens):
    dec = _decoder(D, H, L, 5)
    _randomise_norms(dec, 6)
    tgt, mem, G = _inputs(lens, D, 7)
    ref = _ref_fwd_bwd(lambda m, t, mm: m(t, mm), dec, [tgt, mem], lens, G)
    hip = _hip_decoder(dec, tgt, mem, lens, G, dev, n_heads=H)
    _compare(hip, ref, f"decoder D={D}")


@pytest.mark.parametrize("norm", [True, False], ids=["final_norm", "no_norm"])
@pytest.mark.parametrize("D,lens", [(64, LENS_SMALL), (1024, [1, 65, 320, 321])], ids=["small", "full"])
def test_encoder_stack_vs_torch_fp64(dev, norm, D, lens):
    enc = _encoder(D, 4, 2, 11, norm)
    _randomise_norms(enc, 12)
    x, G = _inputs(lens, D, 13, n=1)
    ref = _ref_fwd_bwd(lambda m, xx: m(xx), enc, [x], lens, G)
    hip = _hip_encoder(enc, x, lens, G, dev)
    _compare(hip, ref, f"encoder D={D} norm={norm}")


def test_decoder_kv_projection_more_layers_than_one_launch(dev):
    """Six layers: the memory's K / V projections take two grouped launches (four layers, then two)."""
    lens = [9, 33]
    dec = _decoder(64, 4, 6, 21)
    tgt, mem, G = _inputs(lens, 64, 22)
    ref = _ref_fwd_bwd(lambda m, t, mm: m(t, mm), dec, [tgt, mem], lens, G)
    _compare(_hip_decoder(dec, tgt, mem, lens, G, dev), ref, "decoder 6 layers")


def test_row_scale(dev):
    from summarizer_amd.autograd import RowScaleFunction
    g = torch.Generator().manual_seed(3)
    x = torch.randn(301, 1024, generator=g, dtype=torch.float64)
    s = torch.rand(301, generator=g, dtype=torch.float64)
    G = torch.randn(301, 1024, generator=g, dtype=torch.float64)
    xd, sd = x.float().to(dev).requires_grad_(True), s.float().to(dev).requires_grad_(True)
    y = RowScaleFunction.apply(xd, sd)
    y.backward(G.float().to(dev))
    xr, sr = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
    (xr * sr[:, None] * G).sum().backward()
    np.testing.assert_allclose(y.detach().cpu().numpy(), (x * s[:, None]).numpy(), atol=1e-6, rtol=0)
    assert rel(xd.grad.cpu().numpy(), xr.grad.numpy()) < 1e-6
    assert rel(sd.grad.cpu().numpy(), sr.grad.numpy()) < 1e-5


def _dropout_run(dev, dec, tgt, mem, lens, G, p, seed):
    return _hip_decoder(dec, tgt, mem, lens, G, dev, opts=dict(layer_eps=1e-5, layer_dropout_p=p, seed=seed))


def test_determinism_and_dropout_masks(dev):
    lens = [65, 200]
    dec = _decoder(128, 4, 2, 31)
    tgt, mem, G = _inputs(lens, 128, 32)
    a = _dropout_run(dev, dec, tgt, mem, lens, G, 0.0, 0)
    b = _dropout_run(dev, dec, tgt, mem, lens, G, 0.0, 0)
    c = _dropout_run(dev, dec, tgt, mem, lens, G, 0.1, 99)
    d = _dropout_run(dev, dec, tgt, mem, lens, G, 0.1, 99)
    e = _dropout_run(dev, dec, tgt, mem, lens, G, 0.1, 100)
    for x, y in ((a, b), (c, d)):              # bit for bit: outputs, input gradients, every weight gradient
        assert np.array_equal(x[0], y[0])
        assert all(np.array_equal(u, v) for u, v in zip(x[1], y[1]))
        assert all(np.array_equal(x[2][n], y[2][n]) for n in x[2])
    assert not np.array_equal(c[0], e[0])      # another seed, other masks
    assert not np.array_equal(a[0], c[0])      # dropout on changes the result
    assert np.isfinite(c[0]).all() and all(np.isfinite(g).all() for g in c[2].values())


def test_dropout_keep_fraction_full_size(dev):
    """The keep fraction of dropout1, read off the output.  The self-attention's out-projection has weight 0 and bias 1 and tgt = 0,
    so norm1's input is the mask itself (0 or 1 / (1 - p) per element); norm1..3 have gain 1 and bias 0, the cross-attention's
    out-projection and linear2 are zero (their dropouts act on zeros).  Every later step keeps the order of a row's two values, so an
    output element is above its row's mean exactly where dropout1 kept it."""
    from summarizer_amd import kernels
    D, lens = 1024, LENS_FULL
    dec = _decoder(D, 4, 1, 41)
    lay = dec.layers[0]
    with torch.no_grad():
        lay.self_attn.out_proj.weight.zero_(); lay.self_attn.out_proj.bias.fill_(1.0)
        lay.multihead_attn.out_proj.weight.zero_(); lay.multihead_attn.out_proj.bias.zero_()
        lay.linear2.weight.zero_(); lay.linear2.bias.zero_()
        for n in (lay.norm1, lay.norm2, lay.norm3):
            n.weight.fill_(1.0); n.bias.zero_()
    names = kernels.tf_decoder_param_names("layers.", 1)
    p = dict(dec.named_parameters())
    ts = [p[n].detach().to(dev).contiguous() for n in names]
    R = sum(lens)
    tgt = torch.zeros(R, D, device=dev)
    mem = torch.randn(R, D, device=dev)
    sb = kernels.SeqBatch.get(lens, dev)
    out, _ = kernels.tf_decoder_forward(tgt, mem, sb, ts, 1, 4, D, dict(layer_eps=1e-5, layer_dropout_p=0.1, seed=1234), training=True)
    kept = (out > out.mean(dim=1, keepdim=True)).float().mean().item()
    assert abs(kept - 0.9) < 0.01, kept


def test_poisoned_workspace(dev, monkeypatch):
    from test_gpu_poison import Poison
    from summarizer_amd import kernels
    lens = [1, 2, 65, 130, 22]
    dec = _decoder(128, 4, 2, 51)
    tgt, mem, G = _inputs(lens, 128, 52)
    clean = _hip_decoder(dec, tgt, mem, lens, G, dev)
    with Poison(monkeypatch):
        kernels._ws_cache.clear()
        dirty = _hip_decoder(dec, tgt, mem, lens, G, dev)
    assert np.array_equal(clean[0], dirty[0])
    assert all(np.array_equal(u, v) for u, v in zip(clean[1], dirty[1]))
    assert all(np.array_equal(clean[2][n], dirty[2][n]) for n in clean[2])


def test_packed_batch_equals_videos_alone(dev):
    lens = [5, 64, 130, 17]
    dec = _decoder(128, 4, 2, 61)
    tgt, mem, G = _inputs(lens, 128, 62)
    y, dins, _ = _hip_decoder(dec, tgt, mem, lens, G, dev)
    off = np.concatenate([[0], np.cumsum(lens)])
    for i, T in enumerate(lens):
        s = slice(off[i], off[i + 1])
        yi, di, _ = _hip_decoder(dec, tgt[s], mem[s], [T], G[s], dev)
        np.testing.assert_allclose(y[s], yi, atol=1e-5, rtol=0, err_msg=f"video {i}")
        for a, b in zip(dins, di):
            np.testing.assert_allclose(a[s], b, atol=1e-5, rtol=1e-4, err_msg=f"video {i} grad")


def test_model_classes_vs_stock_modules(dev):
    """SumGANAtt's selector and autoencoder on HIP against the stock torch modules they hold, in float64 on the CPU."""
    from summarizer_amd.models.sumgan_att import SumGANAtt
    torch.manual_seed(71)
    m = SumGANAtt(input_size=64, s_encoder_layers=2, s_attention_heads=4, ae_encoder_layers=2, ae_attention_heads=4,
                  cLSTM_hidden_size=32, cLSTM_num_layers=2).eval()
    x = torch.randn(40, 1, 64)
    ref = m.double()
    with torch.no_grad():
        s_ref = ref.summarizer.selector.out(ref.summarizer.selector.transformer_encoder(x.double())).numpy()
        enc = ref.summarizer.ae.transformer_encoder(x.double())
        xh_ref = ref.summarizer.ae.transformer_decoder(x.double(), enc).numpy()
    m = m.float().to(dev)
    with torch.no_grad():
        s = m(x.to(dev)).cpu().numpy()
        xh = m.summarizer.ae(x.to(dev)).cpu().numpy()
    np.testing.assert_allclose(s, s_ref, atol=TOL, rtol=0)
    np.testing.assert_allclose(xh, xh_ref, atol=TOL, rtol=0)
    # a training-mode pass with gradients reaches every parameter a forward uses through the HIP backward
    m.train()
    x_hat, scores = m.summarizer(x.to(dev))
    (x_hat.sum() + scores.sum()).backward()
    params = dict(m.summarizer.named_parameters())
    used = [n for n in params if "_layer." not in n]
    assert used and all(params[n].grad is not None and torch.isfinite(params[n].grad).all() for n in used)


def test_module_goldens(dev):
    """tests/golden/sumgan_att.npz (the reference's modules, seeded weights, dropout off): selector scores, autoencoder x_hat, and the
    decoder stack's output, per ragged video."""
    from conftest import load_golden
    from summarizer_amd import kernels
    from summarizer_amd.models.sumgan_att import SumGANAtt
    import recipes as R
    g = load_golden("sumgan_att")
    D, heads, layers, seed = (int(v) for v in g["meta"])
    torch.manual_seed(seed)                  # the reference's seeded weights (their digests: tests/test_sumgan_att_host.py)
    m = SumGANAtt(input_size=D, s_encoder_layers=layers, s_attention_heads=heads, ae_encoder_layers=layers, ae_attention_heads=heads,
                  cLSTM_hidden_size=32, cLSTM_num_layers=layers)
    sd = m.state_dict()
    assert [R.digest({k: sd[k].numpy()}) for k in g["w0keys"]] == list(g["w0sha"])
    m = m.to(dev).eval()
    ae = m.summarizer.ae
    for T in (int(t) for t in g["lens"]):
        with torch.no_grad():
            s = m(torch.from_numpy(g[f"T{T}/x"]).to(dev)).cpu().numpy()
            xh = ae(torch.from_numpy(g[f"T{T}/x"]).to(dev)).cpu().numpy()
            sb = kernels.SeqBatch.get([T], dev)
            dec = ae.decode_packed(torch.from_numpy(g[f"T{T}/tgt"]).to(dev).view(T, D), torch.from_numpy(g[f"T{T}/mem"]).to(dev).view(T, D), sb)
        np.testing.assert_allclose(s, g[f"T{T}/scores"], atol=TOL, rtol=0, err_msg=f"scores T={T}")
        np.testing.assert_allclose(xh, g[f"T{T}/x_hat"], atol=TOL, rtol=0, err_msg=f"x_hat T={T}")
        np.testing.assert_allclose(dec.cpu().numpy(), g[f"T{T}/dec"].reshape(T, D), atol=TOL, rtol=0, err_msg=f"decoder T={T}")


def test_sumgan_att_trainer_reproduces_the_reference_trainer_end_to_end():
    """The REAL reference SumGANAttTrainer (CPU) was run in the build container (tests/golden/make_golden_e2e_sumgan_att.py):
    autoencoder pre-training epoch, then 2 epochs of selector+encoder / decoder / discriminator updates (three Adams, global
    gradient-norm clip over stale gradients included), supervised sparsity, input noise in epoch 0, every dropout 0 -- with
    torch.randn_like / torch.rand replaced by the counter-based recipes.DetRandom.  Fed the same draws, the HIP trainer must start
    from the same weights, consume the same number of draws, follow the same six curves, end at the same weights and report the
    same metrics (the bounds of the SumGAN trainer's end-to-end test)."""
    import random
    import recipes as R
    from conftest import load_golden
    from summarizer_amd.models.sumgan_att import SumGANAttTrainer
    from summarizer_amd.utils.datasets import synthetic_dataset
    from summarizer_amd.utils.hps import make_hps
    g = load_golden("e2e_sumgan_att")
    D, SEED, n, dseed, t0, t1, nu, n_draws = [int(v) for v in g["meta"]]
    ds = synthetic_dataset(n, seed=dseed, D=D, t_range=(t0, t1), n_users=nu)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
    ep = {"input_size": str(D), "s_encoder_layers": "2", "s_attention_heads": "4", "ae_encoder_layers": "2", "ae_attention_heads": "4",
          "cLSTM_hidden_size": "32", "pretrain_ae": "1", "epoch_noise": "1", "sup": True}
    hps = make_hps(ds, [{"train_keys": keys[3:], "test_keys": keys[:3]}], epochs=2, test_every_epochs=1, lr=1e-3,
                   selection_algorithm="rank", extra_params=ep)
    torch.manual_seed(SEED); random.seed(SEED)
    tr = SumGANAttTrainer(hps, hps.splits_files[0]).reset()
    for mod in tr.model.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, nn.MultiheadAttention):
            mod.dropout = 0.0
    sd = tr.model.state_dict()
    assert sorted(sd) == sorted(g["w0keys"])
    for k, sha in zip(g["w0keys"], g["w0sha"]):     # initial weights bit for bit (sha256 of the fp32 bytes)
        assert R.digest({k: sd[k].detach().cpu().numpy()}) == sha, f"initial {k}"
    with R.DetRandom(SEED).patch() as det:
        tr.train(0)
        assert det.n == n_draws
    sc = hps.writer.scalars
    for t in ("Lse", "Ld", "Lc", "D_x", "D_x_hat", "D_x_hat_p"):
        got = [v for _, v in sc[f"synthetic/Fold_1/Train/{t}"]]
        np.testing.assert_allclose(got, g[t], rtol=2e-3, atol=1e-5, err_msg=t)   # (Lc is a difference of near-equal probabilities: atol)
    sd = tr.model.state_dict()
    for i, k in enumerate(g["w0keys"]):            # final weights at the golden's seeded sample indices
        w = sd[k].detach().cpu().numpy().reshape(-1)
        d = float(np.abs(w[R.sample_idx(k, w.size, 256)] - g["w1_sample"][g["w1_off"][i]:g["w1_off"][i + 1]]).max())
        assert d < 2e-3, (k, d)
    np.testing.assert_allclose([v for _, v in sc["synthetic/Fold_1/Test/Correlation"]], g["corr"], atol=2e-2)
    f_avg = [v for _, v in sc["synthetic/Fold_1/Test/F-score_avg"]]; f_max = [v for _, v in sc["synthetic/Fold_1/Test/F-score_max"]]
    np.testing.assert_allclose(f_avg, g["f_avg"], atol=2e-2); np.testing.assert_allclose(f_max, g["f_max"], atol=2e-2)
    tr.model.eval()
    with torch.no_grad():
        for k in keys[:3]:
            s = tr.model(torch.from_numpy(ds[k]["features"][...]).unsqueeze(1).cuda()).squeeze().cpu().numpy()
            np.testing.assert_allclose(s, g[f"scores/{k}"], atol=5e-3)
