"""Positional embeddings on the packed path (csrc/posembed.hip; `max_length` models through score_packed, the trainers' packed
steps, Trainer.test's device tail).

Packing rule: packed videos are batch-size-1 calls of the reference (vasnet.py:106-112, transformer.py:82-88): row off[v] + t gets
table[t].  Kernel checks are bit-exact against torch / the library's own cast and split kernels; the model checks compare a
positional model with a same-weights model WITHOUT positions that is handed x + table[pos] -- the pipeline behind the add is the
same code, so scores and gradients must be bit-equal; one independent check goes against the float64 oracle."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import recipes as R

pytestmark = pytest.mark.gpu

LENS = [1, 2, 37, 64]                # a one-frame video, T == max_length, the longest video last
LENS_MID = [2, 64, 1, 37]            # the longest video in the middle
PLANE_LENS = [1, 130, 97, 64]        # 292 rows: 28 pad rows up to the 320-row pitch, more than the plane path's 256-row minimum
SHAPES = [(64, LENS, 64), (64, LENS_MID, 64), (64, [37], 40), (12, [3, 70], 70), (200, [5, 66, 9], 66)]      # (D, lens, table rows)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pos(lens):
    return torch.from_numpy(np.concatenate([np.arange(T) for T in lens]))


def _rand(shape, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(dev)


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _poisoned(numel, dtype, dev):
    t = torch.empty(numel, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(255)
    return t


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("D,lens,rows", SHAPES)
def test_pos_add_packed_fp32_and_bf16_are_bit_exact(dev, D, lens, rows):
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(lens, dev)
    x, table = _rand((sum(lens), D), 1, dev), _rand((rows, D), 2, dev)
    x0 = x.clone()
    y32, y16, planes = kernels.pos_add_packed(x, sb, table, want_f32=True, want_bf16=True)
    assert planes is None
    want = x0 + table[_pos(lens).to(dev)]
    assert torch.equal(_bytes(y32), _bytes(want))                          # a plain fp32 add
    assert torch.equal(_bytes(x), _bytes(x0))                              # x is never written
    want16 = torch.empty(want.shape, dtype=torch.bfloat16, device=dev)
    kernels.cast_f32_bf16(want, want16)
    assert torch.equal(_bytes(y16), _bytes(want16))                        # the rounding of sumk_cast_f32_bf16
    only16 = kernels.pos_add_packed(x, sb, table, want_f32=False, want_bf16=True)
    assert only16[0] is None and torch.equal(_bytes(only16[1]), _bytes(want16))


@pytest.mark.parametrize("n_planes", [2, 3])
@pytest.mark.parametrize("D,lens", [(256, PLANE_LENS), (64, LENS), (144, [70])])
def test_pos_add_packed_planes_equal_split_planes_of_the_sum(dev, D, lens, n_planes):
    from summarizer_amd import _lib, kernels
    lib = _lib.load()
    sb = kernels.SeqBatch.get(lens, dev)
    x, table = _rand((sum(lens), D), 3, dev), _rand((max(lens), D), 4, dev)
    want32 = x + table[_pos(lens).to(dev)]
    want = kernels.split_planes(want32, n_planes)
    nb = lib.sumk_planes_bytes(sb.n_rows, D, n_planes)
    assert want.numel() == nb
    for with_f32 in (False, True):
        got = _poisoned(nb, torch.uint8, dev)
        got[nb - 8192:].zero_()                                            # only the slack behind the last sub-array is the caller's to clear
        y32 = _poisoned(sb.n_rows * D, torch.float32, dev) if with_f32 else None
        _lib.check(lib.sumk_pos_add_packed(kernels._p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, kernels._p(table), table.shape[0],
                                           kernels._p(y32), None, kernels._p(got), n_planes, kernels._stream()), "sumk_pos_add_packed")
        assert torch.equal(got, want), f"planes differ (fp32 output {with_f32})"
        if with_f32:
            assert torch.equal(_bytes(y32), _bytes(want32))


def test_pos_add_packed_refuses_bad_arguments_and_writes_nothing(dev):
    from summarizer_amd import _lib, kernels
    lib = _lib.load()
    D, lens = 64, LENS
    sb = kernels.SeqBatch.get(lens, dev)
    x, table = _rand((sum(lens), D), 5, dev), _rand((max(lens), D), 6, dev)
    out = _poisoned(sb.n_rows * D, torch.float32, dev)
    before = _bytes(out).clone()

    def call(D_, rows, o32, planes=None, n_planes=0):
        return lib.sumk_pos_add_packed(kernels._p(x), D_, sb.n_seq, sb.off_host_p, sb.off_dev_p, kernels._p(table), rows, kernels._p(o32), None,
                                       kernels._p(planes), n_planes, kernels._stream())
    assert call(D, max(lens) - 1, out) != 0                               # a video one frame longer than the table
    assert b"max_length" in lib.sumk_last_error()
    assert call(6, max(lens), out) != 0                                    # D % 4
    pl = _poisoned(lib.sumk_planes_bytes(sb.n_rows, 64, 2), torch.uint8, dev)
    pl_before = pl.clone()
    assert call(24, max(lens), None, pl, 2) != 0                           # planes: D % 16
    assert call(D, max(lens), None, pl, 4) != 0                            # planes: 2 or 3
    assert call(D, max(lens), None) != 0                                   # no output asked for
    torch.cuda.synchronize(dev)
    assert torch.equal(_bytes(out), before) and torch.equal(pl, pl_before)
    with pytest.raises(_lib.SumkError):
        kernels.pos_add_packed(x, sb, table[:-1].contiguous())
    g = _rand((max(lens), D), 7, dev); g0 = g.clone()
    assert lib.sumk_pos_table_grad(kernels._p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, kernels._p(g), max(lens) - 1, kernels._stream()) != 0
    torch.cuda.synchronize(dev)
    assert torch.equal(_bytes(g), _bytes(g0))


@pytest.mark.parametrize("D,lens,rows", SHAPES)
def test_pos_table_grad_is_the_sequential_sum(dev, D, lens, rows):
    from summarizer_amd import kernels
    sb = kernels.SeqBatch.get(lens, dev)
    rows = rows + 3                                                        # rows at or above the longest video exist
    dx, init = _rand((sum(lens), D), 8, dev), _rand((rows, D), 9, dev)
    acc = init.cpu().clone()                                               # plain fp32 adds in ascending video order: exact on any machine
    for piece in torch.split(dx.cpu(), lens):
        acc[:piece.shape[0]] += piece
    runs = []
    for _ in range(2):
        g = init.clone()
        kernels.pos_table_grad(dx, sb, g)
        runs.append(g)
    assert torch.equal(_bytes(runs[0]), _bytes(acc.to(dev)))               # accumulates onto the non-zero table gradient
    assert torch.equal(_bytes(runs[0]), _bytes(runs[1]))                   # deterministic
    assert torch.equal(_bytes(runs[0][max(lens):]), _bytes(init[max(lens):]))
    zero = torch.zeros_like(init)
    kernels.pos_table_grad(dx, sb, zero)
    acc0 = torch.zeros(rows, D)
    for piece in torch.split(dx.cpu(), lens):
        acc0[:piece.shape[0]] += piece
    assert torch.equal(_bytes(zero), _bytes(acc0.to(dev)))


# ------------------------------------------------------------------------------------------------ models
def _too_long(lens):
    out = list(lens)
    out[out.index(max(out))] += 1
    return out


def _vasnet_pair(dev, D, ML, precision, kind="simple", seed=31):
    """(positional model, same-weights model without positions, the positional table on the device)."""
    from summarizer_amd.models.vasnet import VASNet
    w = R.vasnet_weights(D, seed, max_length=ML if kind == "simple" else None)
    mp = VASNet(input_size=D, max_length=ML, pos_embed=kind, precision=precision)
    mp.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m0 = VASNet(input_size=D, precision=precision)
    m0.load_state_dict({k: torch.from_numpy(v) for k, v in w.items() if k != "pos_embed.weight"})
    mp, m0 = mp.to(dev).eval(), m0.to(dev).eval()
    table = mp.pos_embed.weight.detach() if kind == "simple" else mp.pos_embed.to(dev)
    return mp, m0, table, w


def _tf_pair(dev, D, heads, ML, precision, seed=41):
    from summarizer_amd.models.transformer import Transformer
    w = R.transformer_weights(D, 1, seed, max_length=ML)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    mp = Transformer(input_size=D, encoder_layers=1, attention_heads=heads, max_length=ML, pos_embed="simple")
    mp.load_state_dict(sd, strict=False)
    m0 = Transformer(input_size=D, encoder_layers=1, attention_heads=heads)
    m0.load_state_dict({k: v for k, v in sd.items() if k != "pos_embed.weight"}, strict=False)
    mp.precision = m0.precision = precision
    mp, m0 = mp.to(dev).eval(), m0.to(dev).eval()
    return mp, m0, mp.pos_embed.weight.detach(), w


@pytest.mark.parametrize("precision,D,lens,kind", [("fp32", 64, LENS, "simple"), ("fp32", 64, LENS_MID, "simple"), ("fp32", 64, [37], "simple"),
                                                   ("fp32", 64, LENS, "attention"), ("bf16x6", 256, PLANE_LENS, "simple"),
                                                   ("bf16x3", 256, PLANE_LENS, "simple"), ("bf16x3", 256, PLANE_LENS, "attention")])
def test_vasnet_score_packed_with_positions_equals_the_pre_added_input(dev, precision, D, lens, kind):
    mp, m0, table, _ = _vasnet_pair(dev, D, max(lens), precision, kind)
    x = _rand((sum(lens), D), 32, dev) * 0.5
    x0 = x.clone()
    pre = x + table[_pos(lens).to(dev)]
    with torch.no_grad():
        got, want = mp.score_packed(x, lens), m0.score_packed(pre, lens)
        again = mp.score_packed(x, lens)
    assert torch.equal(_bytes(got), _bytes(want)) and torch.equal(_bytes(again), _bytes(want))
    assert torch.equal(_bytes(x), _bytes(x0)), "score_packed mutated its input"
    y32, planes = x._sumk_pos[1]
    assert (planes is not None) == (precision != "fp32"), "the split precisions take the plane path at this shape"
    with pytest.raises(AssertionError, match="higher length than max_length"):
        mp.score_packed(torch.cat([x, x[:1]]), _too_long(lens))


@pytest.mark.parametrize("precision,D,heads,lens", [("fp32", 64, 2, LENS), ("fp32", 64, 2, LENS_MID), ("fp32", 64, 2, [37]),
                                                    ("bf16x3", 256, 2, PLANE_LENS)])
def test_transformer_score_packed_with_positions_equals_the_pre_added_input(dev, precision, D, heads, lens):
    mp, m0, table, _ = _tf_pair(dev, D, heads, max(lens), precision)
    x = _rand((sum(lens), D), 42, dev) * 0.5
    x0 = x.clone()
    pre = x + table[_pos(lens).to(dev)]
    with torch.no_grad():
        got, want = mp.score_packed(x, lens), m0.score_packed(pre, lens)
    assert torch.equal(_bytes(got), _bytes(want))
    assert torch.equal(_bytes(x), _bytes(x0)), "score_packed mutated its input"


def _train_step(m, x, lens, tgt):
    s = m.score_packed(x, lens)
    ((s - tgt) ** 2).mean().backward()
    return s.detach()


@pytest.mark.parametrize("precision,D", [("fp32", 64), ("bf16", 128)])
def test_vasnet_training_gradients_equal_the_pre_added_input(dev, precision, D):
    """Dropout ON (model.train()); the same torch seed before each model's first training call gives both the same masks."""
    from summarizer_amd.training import FlatAdam
    lens = LENS
    mp, m0, table, _ = _vasnet_pair(dev, D, max(lens), precision)
    mp.train(); m0.train()
    opt = FlatAdam(mp.parameters(), lr=1e-3)
    x, tgt = _rand((sum(lens), D), 33, dev) * 0.5, torch.from_numpy(np.random.default_rng(34).random(sum(lens)).astype(np.float32)).to(dev)
    x0 = x.clone()
    pre = (x + mp.pos_embed.weight.detach()[_pos(lens).to(dev)]).requires_grad_(True)
    opt.zero_grad()
    torch.manual_seed(5); s1 = _train_step(mp, x, lens, tgt)
    torch.manual_seed(5); s0 = _train_step(m0, pre, lens, tgt)
    assert torch.equal(_bytes(s1), _bytes(s0)) and torch.equal(_bytes(x), _bytes(x0))
    g0 = dict(m0.named_parameters())
    for k, p in mp.named_parameters():
        if k != "pos_embed.weight":
            assert float(p.grad.abs().max()) > 0 and torch.equal(_bytes(p.grad), _bytes(g0[k].grad)), k
    got = mp.pos_embed.weight.grad
    acc = torch.zeros(got.shape)
    for piece in torch.split(pre.grad.cpu(), lens):                        # the sequential fp32 sum of that model's dx
        acc[:piece.shape[0]] += piece
    assert float(got.abs().max()) > 0 and torch.equal(_bytes(got), _bytes(acc.to(dev)))
    lo, hi = opt.flat_grad.data_ptr(), opt.flat_grad.data_ptr() + 4 * opt.flat_grad.numel()
    assert lo <= got.data_ptr() < hi, "pos_embed.weight.grad is no longer a view of the flat gradient bucket"


def test_transformer_training_table_gradient_is_the_sequential_sum(dev):
    lens, D = LENS, 64
    mp, m0, table, _ = _tf_pair(dev, D, 2, max(lens), "fp32")
    mp.train(); m0.train()
    x, tgt = _rand((sum(lens), D), 43, dev) * 0.5, torch.from_numpy(np.random.default_rng(44).random(sum(lens)).astype(np.float32)).to(dev)
    pre = (x + table[_pos(lens).to(dev)]).requires_grad_(True)
    torch.manual_seed(6); s1 = _train_step(mp, x, lens, tgt)
    torch.manual_seed(6); s0 = _train_step(m0, pre, lens, tgt)
    assert torch.equal(_bytes(s1), _bytes(s0))
    g0 = dict(m0.named_parameters())
    for k, p in mp.named_parameters():
        if k != "pos_embed.weight" and p.grad is not None:
            assert torch.equal(_bytes(p.grad), _bytes(g0[k].grad)), k
    acc = torch.zeros(mp.pos_embed.weight.shape)
    for piece in torch.split(pre.grad.cpu(), lens):
        acc[:piece.shape[0]] += piece
    assert torch.equal(_bytes(mp.pos_embed.weight.grad), _bytes(acc.to(dev)))


# ------------------------------------------------------------------------------------------------ independent: float64
def test_vasnet_packed_positions_vs_float64_oracle(dev):
    """Scores against oracle.vasnet_np in float64, run per video with pos_table (the project's 1e-4 score gate); the table's gradient
    against the float64 torch port (GTOL of test_gpu_train_full.py)."""
    from oracle import torch_port, vasnet_np
    from test_gpu_vasnet import TOL
    from test_gpu_train_full import GTOL, _rel
    lens, D = LENS_MID, 64
    mp, _, _, w = _vasnet_pair(dev, D, max(lens), "fp32")
    xs = [R.features(T, 1, D, 50 + i) - 0.1 for i, T in enumerate(lens)]
    tg = [np.random.default_rng(60 + i).random((T, 1, 1)) for i, T in enumerate(lens)]
    x = torch.from_numpy(np.concatenate([v[:, 0, :] for v in xs])).to(dev)
    tgt = torch.from_numpy(np.concatenate([t.reshape(-1) for t in tg]).astype(np.float32)).to(dev)
    with torch.no_grad():
        got = mp.score_packed(x, lens).cpu().numpy()
    want = np.concatenate([vasnet_np.vasnet_forward(v, w, pos_table=w["pos_embed.weight"], dtype=np.float64).reshape(-1) for v in xs])
    err = float(np.abs(got - want).max())
    print(f"packed positional scores vs float64 oracle: max|d| = {err:.3e} (gate {TOL})")
    assert err < TOL
    s = mp.score_packed(x, lens)                       # eval mode with gradients: no dropout
    off = np.concatenate([[0], np.cumsum(lens)])
    sum(((s[off[i]:off[i + 1]] - tgt[off[i]:off[i + 1]]) ** 2).mean() for i in range(len(lens))).backward()
    pt = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in w.items()}
    sum(torch.nn.functional.mse_loss(torch_port.vasnet_scores(torch.from_numpy(v).double(), pt, pos_table=pt["pos_embed.weight"]), torch.from_numpy(t))
        for v, t in zip(xs, tg)).backward()
    rel = _rel(mp.pos_embed.weight.grad.cpu().numpy(), pt["pos_embed.weight"].grad.numpy())
    print(f"table gradient vs float64 port: rel = {rel:.3e} (gate {GTOL})")
    assert rel < GTOL


# ------------------------------------------------------------------------------------------------ cache
def test_cached_sum_follows_the_table(dev):
    """Score, one FlatAdam step (a C-ABI write torch's version counter does not see), score again on the SAME x object: the second result
    is what a fresh model with the stepped weights gives; the same after load_state_dict."""
    from summarizer_amd.models.vasnet import VASNet
    from summarizer_amd.training import FlatAdam
    lens, D = PLANE_LENS, 256
    for precision in ("fp32", "bf16x3"):
        mp, _, _, w = _vasnet_pair(dev, D, max(lens), precision)
        w_start = {k: v.detach().clone() for k, v in mp.state_dict().items()}
        opt = FlatAdam(mp.parameters(), lr=1e-2)
        x, tgt = _rand((sum(lens), D), 35, dev) * 0.5, torch.rand(sum(lens), device=dev)

        def fresh_scores():
            m2 = VASNet(input_size=D, max_length=max(lens), precision=precision)
            m2.load_state_dict({k: v.detach().cpu() for k, v in mp.state_dict().items()})
            with torch.no_grad():
                return m2.to(dev).eval().score_packed(x.clone(), lens)
        with torch.no_grad():
            s1 = mp.score_packed(x, lens)
            kept = x._sumk_pos[1][0]
            mp.score_packed(x, lens)
            assert x._sumk_pos[1][0] is kept, "the sum of an unchanged (x, table) is reused"
        opt.zero_grad()
        _train_step(mp, x, lens, tgt)                  # eval mode with gradients
        table_before = mp.pos_embed.weight.detach().clone()
        opt.step()
        assert not torch.equal(table_before, mp.pos_embed.weight.detach())
        with torch.no_grad():
            s2 = mp.score_packed(x, lens)
        assert torch.equal(_bytes(s2), _bytes(fresh_scores())) and not torch.equal(s1, s2)
        mp.load_state_dict(w_start)
        with torch.no_grad():
            s3 = mp.score_packed(x, lens)
        assert torch.equal(_bytes(s3), _bytes(s1)) and torch.equal(_bytes(s3), _bytes(fresh_scores()))


# ------------------------------------------------------------------------------------------------ trainers
def _splits(keys, n_test=3):
    return [{"train_keys": keys[n_test:], "test_keys": keys[:n_test]}]


@pytest.fixture(scope="module")
def data():
    from summarizer_amd.utils.datasets import synthetic_dataset
    ds = synthetic_dataset(8, seed=5, D=128, t_range=(40, 90), n_users=6)
    return ds, sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))


@pytest.mark.parametrize("kind", ["vasnet", "transformer"])
def test_trainer_test_with_max_pos_takes_the_device_tail(data, kind):
    from summarizer_amd.models.transformer import TransformerTrainer
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.hps import make_hps
    ds, keys = data
    extra = {"input_size": "128", "max_pos": "96"}
    if kind == "transformer":
        extra.update(encoder_layers="1", attention_heads="4")
    hps = make_hps(ds, _splits(keys), epochs=1, extra_params=extra, selection_algorithm="knapsack")
    torch.manual_seed(7)
    tr = (VASNetTrainer if kind == "vasnet" else TransformerTrainer)(hps, hps.splits_files[0]).reset()
    assert tr.model.max_length == 96
    tr.model.eval()
    test_keys = keys[:3]
    with torch.no_grad():
        res = tr._test_on_device(test_keys)
        assert res is not None, "a model with max_pos must take the device evaluation tail"
        acts = {k: tr.model(torch.from_numpy(ds[k]["features"][...]).unsqueeze(1).cuda()).squeeze().cpu().numpy() for k in test_keys}
        batched = tr._score_keys(test_keys)
    for k in test_keys:
        assert np.array_equal(acts[k], batched[k]), k                      # packed scoring == the per-video reference interface
    corr, f_avg, f_max, _ = tr._evaluate_native(acts, test_keys)
    np.testing.assert_allclose(res[0], corr, rtol=0, atol=1e-12)           # (the device-tail tests' tolerance: float64, another summation order)
    np.testing.assert_array_equal(res[1], f_avg); np.testing.assert_array_equal(res[2], f_max)
    got = tr.test(0)
    np.testing.assert_allclose(got[0], np.mean(corr), rtol=0, atol=1e-12)
    assert got[1] == (np.mean(f_avg), np.mean(f_max))


def test_vasnet_trainer_with_max_pos_hip_graph_steps_equal_eager_steps(data):
    """Three epochs with the per-video HIP graphs and three eager ones end in bit-identical weights, the positional table included.
    Dropout off, as in test_vasnet_trainer_hip_graph_steps_equal_eager_steps: a replay draws its masks through the device-side seed
    word, an eager step through the host counter, so only a dropout-free run can be compared bit for bit."""
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.hps import make_hps
    ds, keys = data
    runs, captured = {}, {}
    for flag in ("1", "0"):
        hps = make_hps(ds, _splits(keys), epochs=3, test_every_epochs=2, lr=1e-3, extra_params={"input_size": "128", "max_pos": "96", "hip_graph": flag})
        torch.manual_seed(7); random.seed(3)
        tr = VASNetTrainer(hps, hps.splits_files[0]).reset()
        tr.model.dropout.p = 0.0
        n, inner = [0], tr._capture_step

        def counting(*a, _inner=inner, _n=n, **k):
            out = _inner(*a, **k)
            _n[0] += 1
            return out
        tr._capture_step = counting
        random.seed(3)
        best = tr.train(0)
        captured[flag] = n[0]
        runs[flag] = (best, [v for _, v in hps.writer.scalars["synthetic/Fold_1/Train/Loss"]],
                      {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()})
    assert captured["1"] >= 1 and captured["0"] == 0, captured
    assert runs["1"][1] == runs["0"][1] and np.isfinite(runs["1"][1]).all()
    assert "pos_embed.weight" in runs["1"][2]
    for k, v in runs["1"][2].items():
        assert torch.equal(v, runs["0"][2][k]), k


@pytest.mark.parametrize("kind", ["vasnet", "transformer"])
def test_trainers_with_max_pos_train_batched_steps(data, kind):
    from summarizer_amd.models.transformer import TransformerTrainer
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.hps import make_hps
    ds, keys = data
    extra = {"input_size": "128", "max_pos": "96", "batch_videos": "2"}
    if kind == "transformer":
        extra.update(encoder_layers="1", attention_heads="4")
    hps = make_hps(ds, _splits(keys), epochs=2, test_every_epochs=1, lr=5e-4, extra_params=extra)
    torch.manual_seed(1); random.seed(1)
    tr = (VASNetTrainer if kind == "vasnet" else TransformerTrainer)(hps, hps.splits_files[0]).reset()
    t0 = tr.model.pos_embed.weight.detach().cpu().clone()
    best = tr.train(0)
    losses = [v for _, v in hps.writer.scalars["synthetic/Fold_1/Train/Loss"]]
    assert np.isfinite(losses).all() and all(np.isfinite(best))
    assert not torch.equal(t0, tr.model.pos_embed.weight.detach().cpu()), "the positional table did not train"
