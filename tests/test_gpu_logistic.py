"""GPU: the logistic-regression and random baselines on the HIP path.
 * LogisticRegression.forward / score_packed (frame-head kernel) equal the reference's outputs (tests/golden/logistic.npz);
 * sumk_logistic_step (csrc/logistic.hip) equals the existing kernels composed (frame head -> segment MSE mean -> frame-head backward
   -> adam_step_dev), follows the reference's MSELoss + Adam trajectory, is bit-deterministic, its gradient-only mode + FlatAdam.step()
   equals its fused mode bit for bit, and it holds at the grid's block / cap boundaries, on a poisoned workspace and under graph replay;
 * the trainers reproduce the reference trainers end to end (tests/golden/e2e_logistic.npz, e2e_random.npz), and two data-parallel ranks
   equal one process stepping on the same two videos as one batch."""
import os
import random
import socket

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(D, seed):
    from summarizer_amd.models.logistic import LogisticRegression
    torch.manual_seed(seed)
    return LogisticRegression(input_size=D).to(DEV)


def test_forward_matches_reference_small_and_default_size():
    import recipes as R
    g = load_golden("logistic")
    for D in (64, 128):
        m = _model(D, 1000 + D).eval()
        for T in (1, 2, 37, 300):
            for B in (1, 3):
                x = torch.from_numpy(R.features(T, B, D, 10 * T + B)).to(DEV)
                with torch.no_grad():
                    y = m(x).cpu().numpy()
                assert y.shape == (T, B, 1)
                np.testing.assert_allclose(y, g[f"D{D}/T{T}B{B}/y"], atol=1e-6, err_msg=f"D={D} T={T} B={B}")
    m = _model(1024, int(g["D1024/seed"][0])).eval()
    with torch.no_grad():
        y = m(torch.from_numpy(R.features(50, 1, 1024, 3)).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(y, g["D1024/y"], atol=1e-6)


def test_score_packed_ragged_equals_per_video_calls():
    m = _model(128, 3).eval()
    lens = [5, 1, 77, 32]
    xs = [torch.rand(T, 128, device=DEV) for T in lens]
    with torch.no_grad():
        packed = m.score_packed(torch.cat(xs), lens)
        single = torch.cat([m(x.unsqueeze(1)).view(-1) for x in xs])
    torch.testing.assert_close(packed, single, rtol=0, atol=0)


def test_forward_autograd_matches_torch():
    m = _model(64, 4)
    x = torch.rand(20, 2, 64, device=DEV)
    m(x).sum().backward()
    w, b = m.perceptron.weight.detach().clone().requires_grad_(), m.perceptron.bias.detach().clone().requires_grad_()
    torch.sigmoid(x.view(-1, 64) @ w.t() + b).sum().backward()
    torch.testing.assert_close(m.perceptron.weight.grad, w.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m.perceptron.bias.grad, b.grad, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- the step kernel
class Buckets:
    """FlatAdam-shaped buckets of nn.Linear(D, 1): [w (D) | b | 3 pad]."""

    def __init__(self, D, seed=0, lr=1e-2, wd=1e-5):
        from summarizer_amd.training import FlatAdam
        self.m = _model(D, seed)
        self.opt = FlatAdam(self.m.parameters(), lr=lr, weight_decay=wd)

    def step(self, x, sb, t, scale, apply_adam=True, **kw):
        from summarizer_amd import kernels
        o = self.opt
        return kernels.logistic_step(x, sb, t, o.flat_param, o.flat_grad, o.exp_avg, o.exp_avg_sq, o._state, o.lr, o.betas, o.eps,
                                     o.weight_decay, scale, apply_adam=apply_adam, want_scores=True, **kw)

    def state(self):
        o = self.opt
        return [t.detach().cpu().clone() for t in (o.flat_param, o.exp_avg, o.exp_avg_sq, o._state)]


def _batch(lens, D, seed=0):
    from summarizer_amd import kernels
    gen = torch.Generator().manual_seed(seed)
    x = (0.5 * torch.randn(sum(lens), D, generator=gen).abs()).to(DEV)
    t = torch.rand(sum(lens), generator=gen).to(DEV)
    return x, kernels.SeqBatch.get(lens, DEV), t


def _composed_step(bk, x, sb, t, scale):
    """The same step from the existing kernels: frame head, segment MSE mean (+ backward), frame-head backward, adam_step_dev."""
    from summarizer_amd import kernels
    from summarizer_amd.autograd import FrameHeadFunction, SegmentMseMeanFunction
    bk.opt.zero_grad()
    s = FrameHeadFunction.apply(x, bk.m.perceptron.weight, bk.m.perceptron.bias)
    loss = SegmentMseMeanFunction.apply(s, t, sb, scale)
    loss.backward()
    bk.opt.step()
    return loss.detach(), s.detach()


@pytest.mark.parametrize("lens", [[37], [50, 1, 300, 64]])
@pytest.mark.parametrize("D", [128, 1024])
def test_step_equals_composed_kernels(lens, D):
    x, sb, t = _batch(lens, D, 1)
    a, b = Buckets(D, 5), Buckets(D, 5)
    for _ in range(3):
        loss_a, mse_a, s_a = a.step(x, sb, t, 1.0 / len(lens))
        loss_b, s_b = _composed_step(b, x, sb, t, 1.0 / len(lens))
        torch.testing.assert_close(loss_a[0], loss_b, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(s_a, s_b, rtol=0, atol=1e-6)
    ref_mse = torch.stack([((s_b[o0:o1] - t[o0:o1]) ** 2).mean() for o0, o1 in zip(sb.off_host[:-1], sb.off_host[1:])])
    torch.testing.assert_close(mse_a, ref_mse, rtol=1e-5, atol=1e-7)
    sa, sbk = a.state(), b.state()
    for u, v in zip(sa[:3], sbk[:3]):
        torch.testing.assert_close(u, v, rtol=0, atol=1e-6)
    assert torch.equal(sa[3], sbk[3]) and int(sa[3][0]) == 3          # step counters (and the adam scratch words) identical


@pytest.mark.parametrize("name", ["one", "two"])
def test_three_step_trajectory_matches_reference(name):
    import recipes as R
    from summarizer_amd import kernels
    g = load_golden("logistic")
    lr, wd, D = g["traj/meta"]
    D = int(D)
    lens = [int(v) for v in g[f"traj/{name}/lens"]]
    bk = Buckets(D, 7, lr=float(lr), wd=float(wd))
    vids = [R.synthetic_video(T, 40 + i, n_users=2, D=D) for i, T in enumerate(lens)]
    x = torch.from_numpy(np.concatenate([v["features"] for v in vids])).to(DEV)
    ts = []
    for v in vids:
        gt = torch.from_numpy(v["gtscore"].copy()); gt = gt - gt.min(); ts.append(gt / (gt.max() - gt.min()))
    t = torch.cat(ts).to(DEV)
    sb = kernels.SeqBatch.get(lens, DEV)
    for s in range(3):
        loss, _, _ = bk.step(x, sb, t, 1.0 / len(lens))
        np.testing.assert_allclose(loss.cpu().numpy(), g[f"traj/{name}/loss{s}"], rtol=1e-5, atol=1e-6)
        for k, v in bk.m.state_dict().items():
            np.testing.assert_allclose(v.cpu().numpy(), g[f"traj/{name}/w{s}/{k}"], atol=1e-5, err_msg=f"step {s} {k}")


def test_two_identical_calls_are_bitwise_equal():
    lens = [240, 17, 333, 90, 1]
    x, sb, t = _batch(lens, 1024, 2)
    outs = []
    for _ in range(2):
        bk = Buckets(1024, 9)
        loss, mse, s = bk.step(x, sb, t, 0.2)
        outs.append([loss.cpu(), mse.cpu(), s.cpu()] + bk.state())
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_gradient_only_then_flatadam_step_equals_fused_bitwise():
    lens = [64, 128, 7]
    x, sb, t = _batch(lens, 1024, 3)
    fused, split = Buckets(1024, 11), Buckets(1024, 11)
    for _ in range(3):
        lf, _, sf = fused.step(x, sb, t, 1.0 / 3)
        split.opt.zero_grad()
        ls, _, ss = split.step(x, sb, t, 1.0 / 3, apply_adam=False)
        split.opt.step()
        assert torch.equal(lf, ls) and torch.equal(sf, ss)
    for u, v in zip(fused.state(), split.state()):
        assert torch.equal(u, v)


def test_gradient_only_mode_accumulates_into_grad():
    x, sb, t = _batch([50, 20], 128, 4)
    bk = Buckets(128, 2)
    bk.opt.zero_grad()
    p0 = bk.opt.flat_param.clone()
    bk.step(x, sb, t, 0.5, apply_adam=False)
    g1 = bk.opt.flat_grad.clone()
    bk.step(x, sb, t, 0.5, apply_adam=False)
    torch.testing.assert_close(bk.opt.flat_grad, 2 * g1, rtol=1e-6, atol=0)
    assert torch.equal(bk.opt.flat_param, p0) and int(bk.opt._state[0]) == 0
    assert torch.count_nonzero(g1[129:]) == 0


@pytest.mark.parametrize("lens", [[1], [31], [32], [33], [3, 30], [1024], [1025], [20 + (i % 7) * 3 for i in range(64)], [20000],
                                  [300] * 40 + [7] * 27])
def test_block_and_grid_cap_boundaries(lens):
    D = 128 if sum(lens) > 5000 else 256
    x, sb, t = _batch(lens, D, 5)
    a, b = Buckets(D, 6), Buckets(D, 6)
    loss_a, _, s_a = a.step(x, sb, t, 1.0 / len(lens))
    loss_b, s_b = _composed_step(b, x, sb, t, 1.0 / len(lens))
    torch.testing.assert_close(loss_a[0], loss_b, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(s_a, s_b, rtol=0, atol=1e-6)
    for u, v in zip(a.state()[:3], b.state()[:3]):
        torch.testing.assert_close(u, v, rtol=0, atol=1e-6)


def test_poisoned_workspace_and_fresh_tickets_agree():
    from summarizer_amd import kernels
    lens = [300, 45, 2]
    x, sb, t = _batch(lens, 1024, 6)
    nb = kernels.logistic_step_workspace_bytes(sb.n_rows, 1024)
    res = []
    for fill in (0, 255):
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        bk = Buckets(1024, 12)
        outs = [bk.step(x, sb, t, 1.0 / 3, ws=ws) for _ in range(2)]
        res.append([o.cpu() for out in outs for o in out] + bk.state())
    for u, v in zip(*res):
        assert torch.equal(u, v)


def test_captured_steps_replayed_equal_eager_steps():
    from summarizer_amd import kernels
    lens = [120]
    x, sb, t = _batch(lens, 1024, 7)
    nb = kernels.logistic_step_workspace_bytes(sb.n_rows, 1024)
    eager, graph = Buckets(1024, 13), Buckets(1024, 13)
    for _ in range(4):
        le, _, se = eager.step(x, sb, t, 1.0)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV).fill_(255)
    loss = torch.zeros(1, device=DEV); mse = torch.zeros(1, device=DEV); sc = torch.zeros(sb.n_rows, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graph.step(x, sb, t, 1.0, loss=loss, mse=mse, scores=sc, ws=ws)
    for _ in range(4):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, le) and torch.equal(sc, se)
    for u, v in zip(eager.state(), graph.state()):
        assert torch.equal(u, v)


def test_error_paths_name_the_argument():
    import ctypes as C
    from summarizer_amd import _lib, kernels
    lib = _lib.load()
    x, sb, t = _batch([10], 64, 8)
    bk = Buckets(64, 1)
    o = bk.opt
    ws = torch.empty(kernels.logistic_step_workspace_bytes(10, 64), dtype=torch.uint8, device=DEV)
    p = kernels._p
    loss, mse = torch.empty(1, device=DEV), torch.empty(1, device=DEV)

    def call(xp=None, D=64, tp=None, fp=None, gp=None, st=None, adam=1, wsp=None, nws=None):
        rc = lib.sumk_logistic_step(xp if xp is not None else p(x), D, 1, sb.off_host_p, sb.off_dev_p, tp if tp is not None else p(t),
                                    fp if fp is not None else p(o.flat_param), gp if gp is not None else p(o.flat_grad), p(o.exp_avg),
                                    p(o.exp_avg_sq), st if st is not None else p(o._state), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, adam,
                                    p(loss), p(mse), None, wsp if wsp is not None else p(ws), ws.numel() if nws is None else nws,
                                    kernels._stream())
        with pytest.raises(_lib.SumkError) as e:
            _lib.check(rc, "sumk_logistic_step")
        return str(e.value)

    null = C.c_void_p(0)
    assert "x is null" in call(xp=null)
    assert "target is null" in call(tp=null)
    assert "flat_param is null" in call(fp=null)
    assert "state is null" in call(st=null)
    assert "flat_grad is null" in call(gp=null, adam=0)
    assert "workspace is null" in call(wsp=null)
    assert "bad D=62" in call(D=62)
    assert "bad D=4096" in call(D=4096)
    assert "workspace" in call(nws=16) and "required" in call(nws=16)


# ---------------------------------------------------------------- trainers
def _dataset(g):
    from summarizer_amd.utils.datasets import synthetic_dataset
    D, SEED, n, dseed, t0, t1, nu, epochs = [int(v) for v in g["meta"]]
    ds = synthetic_dataset(n, seed=dseed, D=D, t_range=(t0, t1), n_users=nu)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
    return ds, keys, D, SEED, epochs


@pytest.mark.parametrize("hip_graph", ["1", "0"])
def test_logistic_trainer_reproduces_the_reference_trainer(hip_graph):
    from summarizer_amd.models.logistic import LogisticRegressionTrainer
    from summarizer_amd.utils.hps import make_hps
    g = load_golden("e2e_logistic")
    ds, keys, D, SEED, epochs = _dataset(g)
    hps = make_hps(ds, [{"train_keys": keys[3:], "test_keys": keys[:3]}], epochs=epochs, test_every_epochs=1, lr=1e-3,
                   selection_algorithm="rank", extra_params={"input_size": str(D), "hip_graph": hip_graph})
    torch.manual_seed(SEED); random.seed(SEED)
    tr = LogisticRegressionTrainer(hps, hps.splits_files[0]).reset()
    for k, v in tr.model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), g[f"w0/{k}"], err_msg=f"initial {k}")
    best = tr.train(0)
    np.testing.assert_allclose([v for _, v in hps.writer.scalars["synthetic/Fold_1/Train/Loss"]], g["losses"], rtol=1e-5, atol=1e-7)
    for k, v in tr.model.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), g[f"w1/{k}"], atol=1e-5, err_msg=f"final {k}")
    for tag, key in (("corr", "Correlation"), ("f_avg", "F-score_avg"), ("f_max", "F-score_max")):
        np.testing.assert_allclose([v for _, v in hps.writer.scalars[f"synthetic/Fold_1/Test/{key}"]], g[tag], atol=1e-6, err_msg=tag)
    np.testing.assert_allclose(best, g["best"], atol=1e-6)
    assert int(tr.optimizer._state[0]) == epochs * len(keys[3:])


def test_logistic_trainer_rejects_auto_batch():
    from summarizer_amd._lib import SumkError
    from summarizer_amd.models.logistic import LogisticRegressionTrainer
    from summarizer_amd.utils.hps import make_hps
    g = load_golden("e2e_logistic")
    ds, keys, D, SEED, epochs = _dataset(g)
    hps = make_hps(ds, [{"train_keys": keys[3:], "test_keys": keys[:3]}], epochs=1, extra_params={"input_size": str(D), "batch_videos": "auto"})
    tr = LogisticRegressionTrainer(hps, hps.splits_files[0]).reset()
    with pytest.raises(SumkError, match="auto"):
        tr.train(0)


def test_random_trainer_reproduces_the_reference_trainer():
    from summarizer_amd.models.rand import RandomTrainer
    from summarizer_amd.utils.hps import make_hps
    g = load_golden("e2e_random")
    ds, keys, D, SEED, epochs = _dataset(g)
    hps = make_hps(ds, [{"train_keys": keys[3:], "test_keys": keys[:3]}], epochs=epochs, test_every_epochs=1, lr=1e-3,
                   selection_algorithm="rank")
    got = {}
    torch.manual_seed(SEED); random.seed(SEED)
    tr = RandomTrainer(hps, hps.splits_files[0]).reset()
    orig = tr.draw_scores
    tr.draw_scores = lambda fold, d: (got.update(d), orig(fold, d))
    best = tr.train(0)
    for k in keys[3:]:
        np.testing.assert_array_equal(got[k].cpu().numpy().reshape(-1), g[f"train_scores/{k}"], err_msg=k)
    np.testing.assert_allclose([v for _, v in hps.writer.scalars["synthetic/Fold_1/Train/Loss"]], g["losses"], rtol=1e-6)
    for tag, key in (("corr", "Correlation"), ("f_avg", "F-score_avg"), ("f_max", "F-score_max")):
        np.testing.assert_allclose([v for _, v in hps.writer.scalars[f"synthetic/Fold_1/Test/{key}"]], g[tag], atol=1e-6, err_msg=tag)
    np.testing.assert_allclose(best, g["best"], atol=1e-6)
    assert tr.best_weights is not None and len(tr.best_weights) == 0


# ---------------------------------------------------------------- data parallel (2 ranks on one GPU over gloo)
def _run(rank, world, port, q, bv):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from summarizer_amd.models.logistic import LogisticRegressionTrainer
    from summarizer_amd.utils.datasets import synthetic_dataset
    from summarizer_amd.utils.hps import make_hps
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ds = synthetic_dataset(3, seed=9, D=128, t_range=(40, 90), n_users=4)
        keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
        hps = make_hps(ds, [{"train_keys": keys[:2], "test_keys": keys[2:]}], epochs=2, test_every_epochs=5, lr=1e-3,
                       selection_algorithm="rank", extra_params={"input_size": "128", "batch_videos": str(bv)})
        torch.manual_seed(100 + rank)          # DIFFERENT init per rank: broadcast_parameters must make them agree
        random.seed(5)
        tr = LogisticRegressionTrainer(hps, hps.splits_files[0]).reset()
        if world == 1:
            torch.manual_seed(100); tr = LogisticRegressionTrainer(hps, hps.splits_files[0]).reset()
        tr.train(0)
        q.put((rank, {k: v.detach().cpu().numpy() for k, v in tr.model.state_dict().items()}))
    finally:
        if world > 1:
            dist.destroy_process_group()


def _spawn(world, bv):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run, args=(r, world, port, q, bv)) for r in range(world)]
    for p in procs: p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs: p.join(timeout=120)
    return res


def test_dp_two_ranks_equal_single_process_batch_of_two():
    dp = _spawn(2, 1)
    single = _spawn(1, 2)[0]
    for k in dp[0]:
        np.testing.assert_array_equal(dp[0][k], dp[1][k], err_msg=f"ranks disagree on {k}")
        np.testing.assert_allclose(dp[0][k], single[k], atol=2e-6, err_msg=f"DP != single-process batch for {k}")
