"""CPU: pins the oracle (numpy restatements + torch port) against vectors produced by the REAL reference
(tests/golden/make_golden.py).  Tolerances: fp32 restatement vs fp32 reference -> 2e-5 abs on scores in (0,1)."""
import warnings

import numpy as np
import pytest
import torch

import recipes as R
from conftest import load_golden, js
from oracle import vasnet_np, lstm_np, reward_np, eval_np, knapsack_np, torch_port

TOL = 2e-5


def _kw(meta):
    return dict(ignore_self=meta.get("ignore_self", False), aperture=meta.get("attention_aperture"),
                scale=meta.get("scale"), eps=meta.get("epsilon", 1e-6))


def _cases(g, vname):
    return sorted(k.split("/")[-1] for k in g.files if k.startswith(f"{vname}/x/"))


def test_vasnet_small_numpy_and_torch_port():
    g = load_golden("vasnet_small")
    meta = js(g["meta"])
    for vname, m in meta.items():
        w = {k.split("/w/")[1]: g[k] for k in g.files if k.startswith(f"{vname}/w/")}
        pos = None
        if m.get("max_length"):
            pos = w.pop("pos_embed.weight") if m["pos_embed"] == "simple" else g[f"{vname}/pos_table"]
            if m["pos_embed"] == "attention":
                np.testing.assert_allclose(vasnet_np.sinusoid_table(m["max_length"], 64), pos, atol=1e-6)
        for c in _cases(g, vname):
            x, y = g[f"{vname}/x/{c}"], g[f"{vname}/y/{c}"]
            for dt in (np.float32, np.float64):
                yo = vasnet_np.vasnet_forward(x, w, pos_table=pos, pos_kind=m.get("pos_embed", "simple"), dtype=dt, **_kw(m))
                assert yo.shape == y.shape
                np.testing.assert_allclose(yo, y, atol=TOL, rtol=0, equal_nan=True, err_msg=f"{vname} {c} {dt}")
            yt = torch_port.vasnet_scores(torch.from_numpy(x), {k: torch.from_numpy(v) for k, v in w.items()},
                                          pos_table=None if pos is None else torch.from_numpy(pos),
                                          pos_kind=m.get("pos_embed", "simple"), **_kw(m)).numpy()
            np.testing.assert_allclose(yt, y, atol=TOL, rtol=0, equal_nan=True, err_msg=f"torch {vname} {c}")


def test_vasnet_ignore_self_T1_is_nan():
    # all keys masked -> softmax of all -inf -> NaN in the reference; the oracle must agree, not "fix" it
    g = load_golden("vasnet_small")
    assert np.isnan(g["ignore_self/y/T1B1"]).all()


def test_vasnet_intermediates():
    g = load_golden("vasnet_intermediates")
    w = R.vasnet_weights(64, 100)
    y, it = vasnet_np.vasnet_forward(g["x"], w, return_intermediates=True)
    np.testing.assert_allclose(y, g["y"], atol=TOL)
    for a, b in [("Q", "Q"), ("K", "K"), ("V", "V"), ("alpha", "alpha"), ("c", "c"), ("y1", "y1"), ("y2", "y2")]:
        np.testing.assert_allclose(it[a], g[b][0], atol=5e-5, rtol=1e-4, err_msg=a)


def test_vasnet_full_size():
    g = load_golden("vasnet_full")
    n = len([k for k in g.files if k.endswith("/cfg")])
    for ci in range(n):
        cfg = js(g[f"c{ci}/cfg"])
        if cfg["T"] > 320:
            continue
        w = R.vasnet_weights(cfg["D"], cfg["wseed"]); x = R.features(cfg["T"], cfg["B"], cfg["D"], cfg["xseed"])
        assert R.digest(w) == cfg["wdigest"] and R.digest({"x": x}) == cfg["xdigest"]
        kw = cfg["kw"]
        y = vasnet_np.vasnet_forward(x, w, ignore_self=kw.get("ignore_self", False), aperture=kw.get("attention_aperture"))
        np.testing.assert_allclose(y, g[f"c{ci}/y"], atol=TOL, err_msg=str(cfg))


def test_lstm_small():
    g = load_golden("lstm_small")
    for name, fn, L in [("dsn_small", lstm_np.dsn_forward, 1), ("dsn_small_2l", lstm_np.dsn_forward, 2),
                        ("slstm_small", lstm_np.slstm_forward, 2)]:
        w = {k.split("/w/")[1]: g[k] for k in g.files if k.startswith(f"{name}/w/")}
        for c in _cases(g, name):
            y = fn(g[f"{name}/x/{c}"], w, num_layers=L)
            np.testing.assert_allclose(y, g[f"{name}/y/{c}"], atol=TOL, err_msg=f"{name} {c}")
        pref = "rnn." if name.startswith("dsn") else "lstm."
        h = lstm_np.bilstm_forward(g[f"{name}/x/T37B1"], w, pref, L)
        np.testing.assert_allclose(h, g[f"{name}/h/T37B1"], atol=TOL)


def test_lstm_full_dsn():
    g = load_golden("lstm_full")
    cfg = js(g["c1/cfg"])
    w = R.lstm_weights("rnn.", cfg["D"], cfg["H"], cfg["L"], cfg["wseed"], "out.0.")
    assert R.digest(w) == cfg["wdigest"]
    y = lstm_np.dsn_forward(R.features(cfg["T"], 1, cfg["D"], cfg["xseed"]), w)
    np.testing.assert_allclose(y, g["c1/y"], atol=TOL)


def test_reward():
    g = load_golden("reward")
    for ci in range(5):
        for far in (0, 1):
            ref = g[f"c{ci}/reward_far{far}"]
            got = reward_np.compute_reward(g[f"c{ci}/seq"], g[f"c{ci}/actions"], far_sim=bool(far))
            if f"c{ci}/raises_IndexError" in g.files:
                # one pick: the reference crashes (dsn.py:229-230); the oracle defines div=0, rep=exp(-mean d)
                assert np.isfinite(got) and 0 < got <= 0.5
            else:
                np.testing.assert_allclose(got, ref, atol=2e-5, rtol=1e-5)
    assert reward_np.compute_reward(g["c3/seq"], g["c3/actions"]) == 0.0      # zero picks (dsn.py:199-203)


def test_metrics():
    g = load_golden("metrics")
    for ci in range(3):
        T, U, seed = g[f"c{ci}/T_U_seed"]
        v = R.synthetic_video(int(T), int(seed), n_users=int(U))
        sc = g[f"c{ci}/scores"]
        fs = eval_np.upsample(sc, v["n_frames"], v["picks"])
        np.testing.assert_array_equal(fs, g[f"c{ci}/frame_scores"])
        summ = eval_np.generate_summary(sc, v["change_points"], v["n_frames"], v["n_frame_per_seg"].tolist(), v["picks"], 0.15, "rank")
        np.testing.assert_array_equal(summ, g[f"c{ci}/summary_rank"])
        np.testing.assert_allclose(eval_np.evaluate_summary(summ, v["user_summary"]), g[f"c{ci}/fscore"], rtol=1e-12)
        np.testing.assert_allclose(eval_np.evaluate_summary(summ[:-7], v["user_summary"]), g[f"c{ci}/fscore_short"], rtol=1e-12)
        long = np.concatenate([summ, np.ones(5, np.float32)])
        np.testing.assert_allclose(eval_np.evaluate_summary(long, v["user_summary"]), g[f"c{ci}/fscore_long"], rtol=1e-12)
        np.testing.assert_allclose(eval_np.evaluate_scores(fs, v["user_scores"]), g[f"c{ci}/spearman"], rtol=1e-12)


def test_knapsack_value_optimal_vs_bruteforce():
    rng = np.random.default_rng(3)
    for trial in range(60):
        n = int(rng.integers(1, 13))
        vals = rng.random(n).tolist()
        wts = rng.integers(1, 40, n).tolist()
        cap = int(rng.integers(0, 120))
        picks = knapsack_np.knapsack_dp(vals, wts, n, cap)
        v, w = knapsack_np.knapsack_value(vals, wts, picks)
        assert w <= cap
        assert v == knapsack_np.knapsack_bruteforce_value(vals, wts, cap), (vals, wts, cap, picks)


def test_transformer_oracle_vs_reference_goldens():
    from oracle import transformer_np
    g = load_golden("transformer_small")
    meta = js(g["meta"])
    for name, kw in meta.items():
        w = {k.split("/w/")[1]: g[k] for k in g.files if k.startswith(f"{name}/w/")}
        pos = w.get("pos_embed.weight") if kw.get("max_length") else None
        for c in _cases(g, name):
            y = transformer_np.transformer_forward(g[f"{name}/x/{c}"], w, kw["encoder_layers"], kw["attention_heads"],
                                                   eps=kw.get("epsilon", 1e-5), more_residuals=kw.get("more_residuals", False),
                                                   pos_table=pos)
            np.testing.assert_allclose(y, g[f"{name}/y/{c}"], atol=TOL, rtol=0, err_msg=f"{name} {c}")
    g = load_golden("transformer_full")
    cfg = js(g["c1/cfg"])
    w = R.transformer_weights(cfg["D"], cfg["layers"], cfg["wseed"])
    assert R.digest(w) == cfg["wdigest"]
    y = transformer_np.transformer_forward(R.features(cfg["T"], cfg["B"], cfg["D"], cfg["xseed"]), w, cfg["layers"], cfg["heads"])
    np.testing.assert_allclose(y, g["c1/y"], atol=TOL, rtol=0)


def test_c1_summe_fold0_oracle_vs_the_reference_at_size():
    """BASELINE config 1 at size: the oracle (torch port scores, numpy evaluation tail, knapsack restatement) against the REAL
    reference's Trainer.test(fold 0) on S-SumMe (tests/golden/make_golden_c1.py): scores 2e-5, machine summaries bit-exact under both
    selection algorithms, per-video F-scores and Spearman, and the fold means Trainer.test returned."""
    import hashlib, json
    from summarizer_amd.models.vasnet import VASNet
    from summarizer_amd.utils.datasets import synthetic_dataset
    g = load_golden("c1_summe_fold0")
    meta = json.loads(bytes(g["meta"]).decode())
    ds = synthetic_dataset(meta["n_videos"], seed=meta["dataset_seed"], D=meta["D"], t_range=tuple(meta["t_range"]), n_users=meta["n_users"])
    torch.manual_seed(meta["weight_seed"])
    p = {k: v.detach() for k, v in VASNet(input_size=meta["D"]).named_parameters()}
    for k, v in p.items():
        assert hashlib.sha256(np.ascontiguousarray(v.numpy()).tobytes()).digest() == bytes(g[f"wdigest/{k}"]), k
    keys = meta["fold0"]["test_keys"]
    corrs, fs = [], {"rank": [], "knapsack": []}
    torch.set_num_threads(4)
    for k in keys:
        d = ds[k]
        assert hashlib.sha256(np.ascontiguousarray(d["features"][...]).tobytes()).digest() == bytes(g[f"digest/{k}"]), k
        with torch.no_grad():
            y = torch_port.vasnet_scores(torch.from_numpy(d["features"][...]).unsqueeze(1), p)[:, 0, 0].numpy()
        np.testing.assert_allclose(y, g[f"scores/{k}"], atol=TOL, rtol=0)
        n_frames = int(d["n_frames"][()])
        for algo in ("rank", "knapsack"):
            summ = eval_np.generate_summary(y, d["change_points"][...], n_frames, d["n_frame_per_seg"][...].tolist(), d["picks"][...], 0.15, algo)
            np.testing.assert_array_equal(summ, np.unpackbits(g[f"summary_{algo}/{k}"])[:n_frames].astype(np.float32), err_msg=f"{algo} {k}")
            f = eval_np.evaluate_summary(summ, d["user_summary"][...])
            np.testing.assert_allclose(f, g[f"fscore_{algo}/{k}"], rtol=1e-6)
            fs[algo].append(f)
        c = eval_np.evaluate_scores(eval_np.upsample(y, n_frames, d["picks"][...]), d["user_scores"][...])
        np.testing.assert_allclose(c, float(g[f"corr/{k}"]), atol=5e-5)
        corrs.append(c)
    for algo in ("rank", "knapsack"):
        ref = g[f"test_{algo}"]
        np.testing.assert_allclose(np.mean(corrs), ref[0], atol=2e-5)
        np.testing.assert_allclose(np.mean(np.array(fs[algo]), axis=0), ref[1:], rtol=1e-6)


def test_sumgan_lstm_refs_vs_reference_modules():
    """torch_port.lstm_stack_ref / dlstm_ref -- the float64 oracles of tests/test_gpu_sumgan_full.py -- run in float32 on the
    goldens of the REAL reference eLSTM / cLSTM / dLSTM (tests/golden/sumgan_lstm.npz): outputs, and the gradients of the
    golden's scalar loss w.r.t. the input, the initial state and every parameter, within 1e-5."""
    import torch.nn.functional as F
    g = load_golden("sumgan_lstm")

    def close(got, want, what):
        np.testing.assert_allclose(got.detach().numpy(), want, atol=1e-5, rtol=1e-5, err_msg=what)

    def weights(tag):
        return {k.split("/w/")[1]: torch.from_numpy(g[k]).requires_grad_(True) for k in g.files if k.startswith(f"{tag}/w/")}

    def lstm_params(w):
        return {k[len("lstm."):]: v for k, v in w.items() if k.startswith("lstm.")}

    tags = sorted({k.split("/")[0] for k in g.files if "/" in k})
    assert {t.split("_")[0] for t in tags} == {"elstm", "clstm", "dlstm"}
    for tag in tags:
        w = weights(tag)
        names = sorted(w)
        if tag.startswith("dlstm"):
            h0 = torch.from_numpy(g[f"{tag}/h0"]).requires_grad_(True)
            c0 = torch.from_numpy(g[f"{tag}/c0"]).requires_grad_(True)
            T = g[f"{tag}/y"].shape[0]
            y = torch.stack(torch_port.dlstm_ref(lstm_params(w), (w["recons.weight"], w["recons.bias"]), T, h0, c0), dim=1)
            close(y, g[f"{tag}/y"], f"{tag} x_hat")
            grads = torch.autograd.grad((y * torch.from_numpy(g[f"{tag}/cw"])).sum(), [h0, c0] + [w[k] for k in names])
            close(grads[0], g[f"{tag}/dh0"], f"{tag} dh0")
            close(grads[1], g[f"{tag}/dc0"], f"{tag} dc0")
            for k, gr in zip(names, grads[2:]):
                close(gr, g[f"{tag}/g/{k}"], f"{tag} grad {k}")
            continue
        x = torch.from_numpy(g[f"{tag}/x"]).requires_grad_(True)
        outs, (hn, cn) = torch_port.lstm_stack_ref(list(x.unbind(1)), lstm_params(w))
        if tag.startswith("elstm"):
            ys = [F.linear(hn, w["mu.weight"], w["mu.bias"]), F.linear(hn, w["logvar.weight"], w["logvar.bias"]), cn]
        else:
            ys = [torch.sigmoid(F.linear(hn[-1], w["out.0.weight"], w["out.0.bias"])), hn[-1]]
        for i, (o, b) in enumerate(zip(outs, x.unbind(1))):
            close(o[-1], g[f"{tag}/y1"][i] if tag.startswith("clstm") else hn[-1, i].detach().numpy(), f"{tag} out[-1] video {i}")
        loss = 0
        for i, y in enumerate(ys):
            close(y, g[f"{tag}/y{i}"], f"{tag} output {i}")
            loss = loss + (y * torch.from_numpy(g[f"{tag}/cw{i}"])).sum()
        grads = torch.autograd.grad(loss, [x] + [w[k] for k in names])
        close(grads[0], g[f"{tag}/dx"], f"{tag} dx")
        for k, gr in zip(names, grads[1:]):
            close(gr, g[f"{tag}/g/{k}"], f"{tag} grad {k}")


def test_sumgan_lstm_refs_ragged_and_initial_state_vs_nn_lstm():
    """lstm_stack_ref on a ragged batch with an initial state, and dlstm_ref with per-video lengths, against stock
    torch (nn.LSTM on each video alone; the decoder's step loop written with nn.LSTM as the reference module does)."""
    torch.manual_seed(8)
    D, H, L, lens = 12, 10, 2, [5, 1, 9]
    lstm = torch.nn.LSTM(D, H, num_layers=L).double()
    p = dict(lstm.named_parameters())
    xs = [torch.randn(T, D, dtype=torch.float64) for T in lens]
    h0, c0 = torch.randn(L, len(lens), H, dtype=torch.float64), torch.randn(L, len(lens), H, dtype=torch.float64)
    outs, (hn, cn) = torch_port.lstm_stack_ref(xs, p, h0, c0)
    for i, x in enumerate(xs):
        o, (h, c) = lstm(x.unsqueeze(1), (h0[:, i:i + 1].contiguous(), c0[:, i:i + 1].contiguous()))
        torch.testing.assert_close(outs[i], o[:, 0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(hn[:, i], h[:, 0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(cn[:, i], c[:, 0], rtol=1e-12, atol=1e-12)
    dl = torch.nn.LSTM(H, H, num_layers=L).double()
    recons = torch.nn.Linear(H, D).double()
    got = torch_port.dlstm_ref(dict(dl.named_parameters()), (recons.weight, recons.bias), lens, h0, c0)
    raw = torch_port.dlstm_ref(dict(dl.named_parameters()), None, lens, h0, c0)
    for i, T in enumerate(lens):
        x, h, c = torch.zeros(1, 1, H, dtype=torch.float64), h0[:, i:i + 1].contiguous(), c0[:, i:i + 1].contiguous()
        steps = []
        for _ in range(T):
            x, (h, c) = dl(x, (h, c))
            steps.append(x[0, 0])
        steps = torch.stack(steps)
        torch.testing.assert_close(raw[i], steps, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(got[i], torch.flip(recons(steps), (0,)), rtol=1e-12, atol=1e-12)


def _lstm_stack_before_hooks(x_list, params, h0, c0):
    """lstm_stack_ref as it stood before it took gate_math / matmul, op for op (F.linear with the bias inside, torch.sigmoid / torch.tanh)."""
    F = torch.nn.functional
    L, lens = sum(1 for k in params if k.startswith("weight_ih_l")), [int(x.shape[0]) for x in x_list]
    act = torch.tensor([[t < n for n in lens] for t in range(max(lens))]).unsqueeze(-1)
    seq = torch.nn.utils.rnn.pad_sequence(list(x_list))
    hn, cn = [], []
    for l in range(L):
        gx = F.linear(seq, params[f"weight_ih_l{l}"], params[f"bias_ih_l{l}"])
        h, c, outs = h0[l], c0[l], []
        for t in range(max(lens)):
            i, f, g, o = (gx[t] + F.linear(h, params[f"weight_hh_l{l}"], params[f"bias_hh_l{l}"])).chunk(4, dim=-1)
            cs = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            hs = torch.sigmoid(o) * torch.tanh(cs)
            h, c = torch.where(act[t], hs, h), torch.where(act[t], cs, c)
            outs.append(h)
        seq = torch.stack(outs)
        hn.append(h); cn.append(c)
    return [seq[:n, b] for b, n in enumerate(lens)], (torch.stack(hn), torch.stack(cn))


def _dlstm_before_hooks(params, lens, h0, c0):
    """dlstm_ref(recons=None) as it stood before it took gate_math / matmul, op for op."""
    F = torch.nn.functional
    L, B, H = h0.shape
    x, h, c, outs = h0.new_zeros(B, H), list(h0.unbind(0)), list(c0.unbind(0)), []
    for t in range(max(lens)):
        for l in range(L):
            gx = F.linear(x, params[f"weight_ih_l{l}"], params[f"bias_ih_l{l}"])
            i, f, g, o = (gx + F.linear(h[l], params[f"weight_hh_l{l}"], params[f"bias_hh_l{l}"])).chunk(4, dim=-1)
            c[l] = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
            h[l] = torch.sigmoid(o) * torch.tanh(c[l])
            x = h[l]
        outs.append(x)
    seq = torch.stack(outs)
    return [seq[:n, b] for b, n in enumerate(lens)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_sumgan_lstm_refs_hooks_keep_the_defaults_bit_for_bit(dtype):
    """lstm_stack_ref / dlstm_ref with gate_math / matmul (the hooks of tests/test_gpu_sumgan_lstm_f64.py): with the defaults, outputs,
    final states and every gradient of a ragged batch with h0 / c0 are BIT-identical to the functions as they stood before the hooks
    (restated above), in float64 and in float32, and in float64 still equal nn.LSTM to 1e-12.  Each gate_math is the same function (1e-12
    in float64); a plain-product hook and the one-accumulator dX product (LinearChainDx) change the summation order only; Linear3 on the
    input projection with LinearDw3 on the recurrent product make the bf16x3 roundings (2^-16 relative, not more) and nothing else."""
    torch.manual_seed(18)
    D, H, L, lens = 12, 10, 2, [5, 1, 9, 5, 2]
    lstm = torch.nn.LSTM(D, H, num_layers=L).to(dtype)
    dl = torch.nn.LSTM(H, H, num_layers=L).to(dtype)
    p, pd = dict(lstm.named_parameters()), dict(dl.named_parameters())
    xs = [torch.randn(T, D, dtype=dtype, requires_grad=True) for T in lens]
    h0 = torch.randn(L, len(lens), H, dtype=dtype, requires_grad=True)
    c0 = torch.randn(L, len(lens), H, dtype=dtype, requires_grad=True)
    cw = [torch.randn(T, H, dtype=dtype) for T in lens]
    cwh, cwc = torch.randn(L, len(lens), H, dtype=dtype), torch.randn(L, len(lens), H, dtype=dtype)

    def stack(fn, **kw):
        outs, (hn, cn) = fn(xs, p, h0, c0, **kw)
        leaves = xs + [h0, c0] + list(p.values())
        g = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, cw)) + (hn * cwh).sum() + (cn * cwc).sum(), leaves)
        return [o.detach() for o in outs] + [hn.detach(), cn.detach()] + list(g)

    def dec(fn, **kw):
        outs = fn(pd, lens, h0, c0, **kw)
        g = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, cw)), [h0, c0] + list(pd.values()))
        return [o.detach() for o in outs] + list(g)

    s_old, s_new = stack(_lstm_stack_before_hooks), stack(torch_port.lstm_stack_ref)
    d_old, d_new = dec(_dlstm_before_hooks), dec(lambda q, n, h, c, **kw: torch_port.dlstm_ref(q, None, n, h, c, **kw))
    assert len(s_old) == len(s_new) and all(torch.equal(a, b) for a, b in zip(s_old, s_new))
    assert len(d_old) == len(d_new) and all(torch.equal(a, b) for a, b in zip(d_old, d_new))
    if dtype != torch.float64:
        return
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=0, atol=1e-12)
    for i, x in enumerate(xs):
        o, (h, c) = lstm(x.unsqueeze(1), (h0[:, i:i + 1].contiguous(), c0[:, i:i + 1].contiguous()))
        close(s_new[i], o[:, 0].detach()); close(s_new[len(lens)][:, i], h[:, 0].detach()); close(s_new[len(lens) + 1][:, i], c[:, 0].detach())
    lo = []
    torch_port.lstm_stack_ref(xs, p, h0, c0, layer_outs=lo)
    assert len(lo) == L and all(torch.equal(a.detach(), b) for a, b in zip(lo[-1], s_new))
    plain = lambda a, w, site: a @ w.t()
    chain = lambda a, w, site: torch_port.LinearChainDx.apply(a, w) if site == "ih" else a @ w.t()
    for kw in (dict(gate_math="rcp_form"), dict(gate_math="rcp_sigmoid"), dict(matmul=plain), dict(gate_math="rcp_sigmoid", matmul=chain)):
        for a, b in zip(stack(torch_port.lstm_stack_ref, **kw), s_new):
            close(a, b)
        for a, b in zip(dec(lambda q, n, h, c, **k2: torch_port.dlstm_ref(q, None, n, h, c, **k2), **kw), d_new):
            close(a, b)
    x3 = lambda a, w, site: torch_port.Linear3.apply(a, w, False) if site == "ih" else torch_port.LinearDw3.apply(a, w)
    for got, want in ((stack(torch_port.lstm_stack_ref, matmul=x3), s_new),
                      (dec(lambda q, n, h, c, **k2: torch_port.dlstm_ref(q, None, n, h, c, **k2), matmul=x3), d_new)):
        rel = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want))
        assert 0 < rel < 1e-3, rel                                                            # the roundings happen, and stay at 2^-16


def test_bilstm_stack_ref_vs_nn_lstm_float64():
    """bilstm_stack_ref (the float64 reference of tests/test_gpu_lstm_f64.py) against stock nn.LSTM(bidirectional=True).double()
    through pack_sequence: a ragged batch with a one-frame video and a tie in length, two layers; hidden states of the top layer
    (and of layer 0 against a one-layer module carrying the same weights), scores of a Linear(2H, 1) + sigmoid head, and the
    gradient of a random-weighted sum of the scores w.r.t. every parameter and the inputs, all to 1e-12.  gate_math="rcp_form"
    is the same function: 1e-12 in float64 too.  The bf16x3 hook (Linear3) differs from the plain product by 2^-16 relative, not
    more, forward and backward; the one-accumulator dX product (mm_chain, LinearChainDx) is the plain product in another order."""
    from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence
    torch.manual_seed(9)
    D, H, L, lens = 12, 10, 2, [5, 1, 9, 5, 2]
    lstm = torch.nn.LSTM(D, H, num_layers=L, bidirectional=True).double()
    head = torch.nn.Linear(2 * H, 1).double()
    p = dict(lstm.named_parameters())
    xs = [torch.randn(T, D, dtype=torch.float64, requires_grad=True) for T in lens]
    cw = [torch.randn(T, dtype=torch.float64) for T in lens]
    leaves = xs + list(p.values()) + [head.weight, head.bias]
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=0, atol=1e-12)

    out, _ = pad_packed_sequence(lstm(pack_sequence(xs, enforce_sorted=False))[0])            # (T_max, B, 2H)
    want_h = [out[:T, i] for i, T in enumerate(lens)]
    want_s = [torch.sigmoid(head(h))[:, 0] for h in want_h]
    want_g = torch.autograd.grad(sum((s * w).sum() for s, w in zip(want_s, cw)), leaves)
    l0 = torch.nn.LSTM(D, H, num_layers=1, bidirectional=True).double()
    l0.load_state_dict({k: v for k, v in lstm.state_dict().items() if k.split("_reverse")[0].endswith("_l0")})
    out0, _ = pad_packed_sequence(l0(pack_sequence(xs, enforce_sorted=False))[0])

    for gate_math in ("exact", "rcp_form"):
        layers = torch_port.bilstm_stack_ref(xs, p, gate_math=gate_math)
        assert len(layers) == L and all(len(v) == len(lens) for v in layers)
        got_s = [torch.sigmoid(head(h))[:, 0] for h in layers[-1]]
        got_g = torch.autograd.grad(sum((s * w).sum() for s, w in zip(got_s, cw)), leaves)
        for i, T in enumerate(lens):
            assert tuple(layers[0][i].shape) == tuple(layers[1][i].shape) == (T, 2 * H)
            close(layers[1][i], want_h[i]); close(layers[0][i], out0[:T, i]); close(got_s[i], want_s[i])
        for a, b in zip(got_g, want_g):
            close(a, b)

    hook = lambda a, w, site: torch_port.Linear3.apply(a, w, site == "hh")
    layers3 = torch_port.bilstm_stack_ref(xs, p, matmul=hook)
    got3 = torch.autograd.grad(sum((torch.sigmoid(head(h))[:, 0] * w).sum() for h, w in zip(layers3[-1], cw)), leaves)
    dh = max(float((a - b).detach().abs().max()) for a, b in zip(layers3[-1], want_h))
    dg = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got3, want_g))
    assert 0 < dh < 1e-4 and 0 < dg < 1e-3, (dh, dg)                                          # the roundings happen, and stay at 2^-16

    # the one-accumulator product of the fp32 yardstick's dX GEMM: the same product (K % 8 != 0 included), another order
    a, b = torch.randn(7, 45, dtype=torch.float64), torch.randn(45, 6, dtype=torch.float64)
    close(torch_port.mm_chain(a, b), a @ b)
    a32, b32 = torch.randn(5, 4096), torch.randn(4096, 3)
    e_chain = float((torch_port.mm_chain(a32, b32).double() - a32.double() @ b32.double()).abs().max())
    assert 0 < e_chain < 4096 * 2.0 ** -24 * float((a32.abs() @ b32.abs()).max())              # fp32 roundings, within the chain's bound
    chain = lambda x_, w_, site: torch_port.LinearChainDx.apply(x_, w_) if site == "ih" else x_ @ w_.t()
    layers_c = torch_port.bilstm_stack_ref(xs, p, matmul=chain)
    got_c = torch.autograd.grad(sum((torch.sigmoid(head(h))[:, 0] * w).sum() for h, w in zip(layers_c[-1], cw)), leaves)
    for a, b in zip(got_c, want_g):
        close(a, b)


def test_bigru_stack_ref_vs_nn_gru_float64():
    """bigru_stack_ref (the float64 reference of tests/test_gpu_gru_f64.py) against make_gru(dtype=float64) -- stock
    nn.GRU(bidirectional=True) in float64 -- through pack_sequence: a ragged batch with a one-frame video and a tie in length, two
    layers; hidden states of the top layer (and of layer 0 against a one-layer module carrying the same weights), scores of a
    Linear(2H, 1) + sigmoid head, and the gradient of a random-weighted sum of the scores w.r.t. every parameter and the inputs, all to
    1e-12.  gate_math="rcp_form" is the same function.  The bf16x3 hooks differ from the plain product by 2^-16 relative, not more:
    Linear3 everywhere (the step path), and LinearDw3 on the recurrent product (the persistent path: only dW_hh moves, every forward
    value and every other gradient's recurrent part stays exact).  The one-accumulator dX product is the plain product in another order."""
    from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence
    torch.manual_seed(19)
    D, H, L, lens = 12, 10, 2, [5, 1, 9, 5, 2]
    sd = {f"rnn.{k}": v.detach() for k, v in torch.nn.GRU(D, H, num_layers=L, bidirectional=True).state_dict().items()}
    gru = torch_port.make_gru(sd, "rnn.", D, H, L, dtype=torch.float64)
    head = torch.nn.Linear(2 * H, 1).double()
    p = dict(gru.named_parameters())
    assert all(v.dtype == torch.float64 for v in p.values())
    xs = [torch.randn(T, D, dtype=torch.float64, requires_grad=True) for T in lens]
    cw = [torch.randn(T, dtype=torch.float64) for T in lens]
    leaves = xs + list(p.values()) + [head.weight, head.bias]
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=0, atol=1e-12)
    grads = lambda layers: torch.autograd.grad(sum((torch.sigmoid(head(h))[:, 0] * w).sum() for h, w in zip(layers[-1], cw)), leaves)

    out, _ = pad_packed_sequence(gru(pack_sequence(xs, enforce_sorted=False))[0])             # (T_max, B, 2H)
    want_h = [out[:T, i] for i, T in enumerate(lens)]
    want_s = [torch.sigmoid(head(h))[:, 0] for h in want_h]
    want_g = torch.autograd.grad(sum((s * w).sum() for s, w in zip(want_s, cw)), leaves)
    l0 = torch_port.make_gru({k: v for k, v in sd.items() if k.split("_reverse")[0].endswith("_l0")}, "rnn.", D, H, 1, dtype=torch.float64)
    out0, _ = pad_packed_sequence(l0(pack_sequence(xs, enforce_sorted=False))[0])

    for gate_math in ("exact", "rcp_form"):
        layers = torch_port.bigru_stack_ref(xs, p, gate_math=gate_math)
        assert len(layers) == L and all(len(v) == len(lens) for v in layers)
        for i, T in enumerate(lens):
            assert tuple(layers[0][i].shape) == tuple(layers[1][i].shape) == (T, 2 * H)
            close(layers[1][i], want_h[i]); close(layers[0][i], out0[:T, i]); close(torch.sigmoid(head(layers[1][i]))[:, 0], want_s[i])
        for a, b in zip(grads(layers), want_g):
            close(a, b)

    rel = lambda got: {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip([f"x{i}" for i in range(len(xs))] + list(p) + ["hw", "hb"], got, want_g)}
    layers3 = torch_port.bigru_stack_ref(xs, p, matmul=lambda a, w, site: torch_port.Linear3.apply(a, w, False))
    dh = max(float((a - b).detach().abs().max()) for a, b in zip(layers3[-1], want_h))
    dg = max(rel(grads(layers3)).values())
    assert 0 < dh < 1e-4 and 0 < dg < 1e-3, (dh, dg)                                          # the roundings happen, and stay at 2^-16

    dw3 = lambda a, w, site: torch_port.LinearDw3.apply(a, w) if site == "hh" else a @ w.t()
    layers_w = torch_port.bigru_stack_ref(xs, p, matmul=dw3)
    for a, b in zip(layers_w[-1], want_h):
        close(a, b)                                                                           # the forward is untouched
    rw = rel(grads(layers_w))
    # the weight_hh gradients of both layers carry the bf16x3 rounding and nothing else does (a weight gradient feeds no other gradient)
    assert all((0 < v < 1e-3) if "weight_hh" in k else v < 1e-12 for k, v in rw.items()), rw

    chain = lambda x_, w_, site: torch_port.LinearChainDx.apply(x_, w_) if site == "ih" else x_ @ w_.t()
    for a, b in zip(grads(torch_port.bigru_stack_ref(xs, p, matmul=chain)), want_g):
        close(a, b)


def test_make_gru_float64():
    torch.manual_seed(2)
    m = torch.nn.GRU(6, 5, num_layers=2, bidirectional=True)
    p = {f"rnn.{k}": v.detach() for k, v in m.state_dict().items()}
    g64 = torch_port.make_gru(p, "rnn.", 6, 5, 2, dtype=torch.float64)
    assert all(v.dtype == torch.float64 for v in g64.parameters())
    x = torch.randn(7, 1, 6)
    torch.testing.assert_close(g64(x.double())[0].float(), m(x)[0], rtol=0, atol=1e-6)


def _tf_params(w, dtype=torch.float64):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in w.items()}


def test_transformer_ref_vs_reference_goldens():
    """torch_port.transformer_ref (float64, ragged list API) against the REAL reference: every transformer_small config (B > 1 and
    the 'simple' table included) at the file's tolerance; the transformer_train step's loss and every grad0 entry through float64
    autograd (relative to the tensor's largest entry; the key-bias slice of in_proj_bias is rounding noise of a zero gradient in
    the golden, so it is compared against the whole vector's scale like every other entry)."""
    g = load_golden("transformer_small")
    meta = js(g["meta"])
    assert set(meta) == {"small", "small_res", "small_pos"}
    for name, kw in meta.items():
        w = {k.split("/w/")[1]: g[k] for k in g.files if k.startswith(f"{name}/w/")}
        p = _tf_params(w)
        for c in _cases(g, name):
            x = torch.from_numpy(g[f"{name}/x/{c}"]).double()
            T, B, D = x.shape
            pos = (p["pos_embed.weight"], np.tile(np.arange(T), B)) if kw.get("max_length") else None
            s, u = torch_port.transformer_ref([x[:, b] for b in range(B)], p, kw["encoder_layers"], kw["attention_heads"],
                                              final_eps=kw.get("epsilon", 1e-5), more_residuals=kw.get("more_residuals", False), pos=pos)
            assert torch.allclose(torch.sigmoid(u), s)
            y = s.view(B, T).t().unsqueeze(-1).numpy()
            np.testing.assert_allclose(y, g[f"{name}/y/{c}"], atol=TOL, rtol=0, err_msg=f"{name} {c}")
    g = load_golden("transformer_train")
    for tag, kw in {"tf": dict(layers=2, heads=4), "tf_res": dict(layers=1, heads=8, more_residuals=True)}.items():
        w = {k.split("/w/")[1]: g[k] for k in g.files if k.startswith(f"{tag}/w/")}
        p = {k: v.requires_grad_(True) for k, v in _tf_params(w).items()}
        x = torch.from_numpy(g["x"]).double()[:, 0]
        s, _ = torch_port.transformer_ref([x], p, kw["layers"], kw["heads"], more_residuals=kw.get("more_residuals", False))
        loss = ((s - torch.from_numpy(g["target"]).double().view(-1)) ** 2).mean()
        loss.backward()
        np.testing.assert_allclose(loss.item(), g[f"{tag}/loss0"], rtol=2e-5)
        keys = [k.split("/grad0/")[1] for k in g.files if k.startswith(f"{tag}/grad0/")]
        assert len(keys) == 12 * kw["layers"] + 6, keys
        for k in keys:
            ref = g[f"{tag}/grad0/{k}"]
            got = p[k].grad.numpy()
            assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), (tag, k, np.abs(got - ref).max(), np.abs(ref).max())


def test_transformer_ref_vs_transformer_port_ragged():
    """transformer_ref against the nn.TransformerEncoder-based TransformerPort, both float64, dropout off: a ragged list (each video
    through the port on its own), more_residuals and a 'simple' positional table (row t of every video).  Scores, and the gradients of
    every parameter, of the table and of x."""
    D, L, H = 128, 2, 4
    lens = [1, 5, 33, 64]
    w = R.transformer_weights(D, L, 77, max_length=64)
    port = torch_port.TransformerPort(D, L, H, max_length=64, more_residuals=True).double()
    port.load_state_dict(_tf_params(w))
    port.eval()
    rng = np.random.default_rng(3)
    xs = [torch.from_numpy(rng.standard_normal((T, D)) * 0.5).requires_grad_(True) for T in lens]
    cw = torch.from_numpy(rng.standard_normal(sum(lens)))
    p = {k: v.detach().clone().requires_grad_(True) for k, v in port.state_dict().items()}
    rows = np.concatenate([np.arange(T) for T in lens])
    s, u = torch_port.transformer_ref(xs, p, L, H, more_residuals=True, pos=(p["pos_embed.weight"], rows))
    (s * cw).sum().backward()
    xs2 = [x.detach().clone().requires_grad_(True) for x in xs]
    s2 = torch.cat([port(x.unsqueeze(1))[:, 0, 0] for x in xs2])
    (s2 * cw).sum().backward()
    assert float((s - s2).detach().abs().max()) < 1e-12
    named = dict(port.named_parameters())
    for k, v in named.items():
        if k.startswith("transformer_encoder.norm."):
            continue                                            # the shared LN: the same Parameter as layer_norm.*
        ref = v.grad
        assert ref is not None and float((p[k].grad - ref).abs().max()) <= 1e-10 * max(float(ref.abs().max()), 1e-30), k
    for a, b in zip(xs, xs2):
        assert float((a.grad - b.grad).abs().max()) <= 1e-10 * float(b.grad.abs().max())


def test_transformer_drop_masks_recipe():
    """recipes.transformer_drop_masks: keep fraction of every site within 5 sigma of 1 - p (binomial) at p = 0.1 and 0.5, kept entries
    scaled by 1 / (1 - p), shapes as transformer_ref takes them, and no two sites (or layers) with the same mask."""
    lens, D, Fd, H, L = [1, 37, 200], 64, 96, 4, 2
    for p in (0.1, 0.5):
        m = R.transformer_drop_masks(12345, p, p, lens, D, Fd, H, L)
        sc = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        flat = {}
        for l in range(L):
            assert [a.shape for a in m["attn"][l]] == [(H, T, T) for T in lens]
            flat[f"attn{l}"] = np.concatenate([a.ravel() for a in m["attn"][l]])
            for k, N in (("out", D), ("ff1", Fd), ("ff2", D)):
                assert m[k][l].shape == (sum(lens), N)
                flat[f"{k}{l}"] = m[k][l].ravel()
        assert m["head"].shape == (sum(lens), D)
        flat["head"] = m["head"].ravel()
        for k, a in flat.items():
            assert set(np.unique(a)) <= {np.float32(0), sc}, k
            frac = float((a != 0).mean())
            assert abs(frac - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / a.size), (k, p, frac)
        ks = sorted(flat)
        for i, a in enumerate(ks):
            for b in ks[i + 1:]:
                n = min(flat[a].size, flat[b].size)
                assert not np.array_equal(flat[a][:n] != 0, flat[b][:n] != 0), (a, b)
    # seed and index conventions: another seed draws other masks; the attention index of (row, h, j) is ((row*heads + h) << 20) | j
    m0 = R.transformer_drop_masks(1, 0.5, 0.5, lens, D, Fd, H, L)
    m1 = R.transformer_drop_masks(2, 0.5, 0.5, lens, D, Fd, H, L)
    assert not np.array_equal(m0["head"], m1["head"])
    row, h, j = 1 + 5, 3, 7                                   # video 1, frame 5
    keep = R.dropout_keep(1, 10, np.array([((row * H + h) << 20) | j], dtype=np.uint64), 0.5)[0]
    assert (m0["attn"][1][1][h, 5, j] != 0) == keep
    keep = R.dropout_keep(1, 12, np.array([row * Fd + 9], dtype=np.uint64), 0.5)[0]
    assert (m0["ff1"][1][row, 9] != 0) == keep


# ------------------------------------------------------------------------------------------------ optimiser step: float64 restatement vs stock torch
@pytest.mark.parametrize("weight_decay", [0.0, 1e-5])
@pytest.mark.parametrize("case", ["clip_bites", "clip_idle", "grad_scale_eighth", "no_clip"])
def test_adam_f64_restatement_vs_torch_adam_and_clip_grad_norm(case, weight_decay):
    """oracle/optim_np.AdamF64 against torch.optim.Adam + torch.nn.utils.clip_grad_norm_ in float64 on the CPU, 5 steps: the gradient is
    scaled first (the 1/world of a data-parallel mean), then clipped on the norm of the scaled gradient, then stepped."""
    from oracle import optim_np
    n, lr = 1237, 5e-3
    rng = np.random.default_rng(77)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 0.3 for _ in range(5)]                      # norm of each ~ 0.3 sqrt(1237) = 10.5
    grad_scale, max_norm = {"clip_bites": (1.0, 5.0), "clip_idle": (1.0, 50.0), "grad_scale_eighth": (0.125, 5.0), "no_clip": (0.5, None)}[case]
    ref = optim_np.AdamF64(p0, lr, weight_decay=weight_decay)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr, weight_decay=weight_decay)
    for g in grads:
        coef = ref.step(g, grad_scale=grad_scale, max_norm=max_norm)
        tp.grad = torch.from_numpy(g * grad_scale)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        # the case is what its name says (decided by the float64 norm of the scaled gradient)
        norm = float(np.linalg.norm(g * grad_scale))
        assert {"clip_bites": norm > 2 * max_norm if max_norm else False, "clip_idle": coef == 1.0 and norm < max_norm if max_norm else False,
                "grad_scale_eighth": coef == 1.0 and norm < max_norm < norm * 8 if max_norm else False, "no_clip": coef == 1.0}[case]
        st = opt.state[tp]
        for name, got, want in (("param", ref.p, tp.detach().numpy()), ("exp_avg", ref.m, st["exp_avg"].numpy()),
                                ("exp_avg_sq", ref.v, st["exp_avg_sq"].numpy())):
            # float64 rounding: a handful of operations per element in another order (torch: lerp for m, addcdiv of m by sqrt(v)/sqrt(bc2) + eps).
            # Each element is a sum of two terms that may cancel (b1 m + (1 - b1) g near 0), so its error is a few float64 ulps of the
            # TERMS, not of the result: 4 ulps of the buffer's largest magnitude absolute, next to 1e-13 relative
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=4 * 2.0 ** -53 * np.abs(want).max(), err_msg=f"{case} {name} step {ref.t}")
        assert ref.t == int(st["step"])
    assert optim_np.clip_coef(np.zeros(5), 1.0, 5.0) == 1.0                      # 5 / (0 + 1e-6) clamped: no NaN from a zero gradient


# ------------------------------------------------------------------------------------------------ evaluation edges: host tail vs the numpy oracle
_EDGE_PRESENT = {
    "picks_from_7": lambda v: v["picks"][0] == 7,
    "picks_from_15": lambda v: v["picks"][0] == 15,
    "last_pick_is_n_frames": lambda v: v["picks"][-1] == v["n_frames"] and len(v["picks"]) == v["n_steps"] + 1,
    "repeated_picks": lambda v: sorted(np.unique(v["picks"], return_counts=True)[1].tolist())[-2:] == [2, 3],
    "one_more_interval": lambda v: v["picks"][-1] != v["n_frames"] and len(v["picks"]) == v["n_steps"] + 1,
    "cps_start_below_0": lambda v: v["change_points"][0, 0] < 0,
    "cps_end_past_video": lambda v: v["change_points"][-1, 1] > v["n_frames"] - 1,
    "segment_lengths": lambda v: (v["n_frame_per_seg"][:8].tolist() == [1, 7, 8, 9, 128, 129, 257, 1100]
                                  and (v["n_frame_per_seg"] < 8).any()),
    "pick_spacing_2": lambda v: (np.diff(v["picks"][:v["n_steps"]]) == 2).all() and v["n_steps"] >= 4000 and v["n_frames"] < 8300,
    "n_frames_1": lambda v: v["n_frames"] == 1,
    "n_frames_5": lambda v: v["n_frames"] == 5 and v["n_steps"] == 2,
    "n_frames_9": lambda v: v["n_frames"] == 9 and v["n_steps"] == 3,
}


def test_every_evaluation_edge_is_present_in_its_video():
    assert set(_EDGE_PRESENT) == set(R.EVAL_EDGES)
    base = R.synthetic_video(130, 5, n_users=3)
    assert base["picks"][0] == 0 and base["picks"][-1] != base["n_frames"] and len(base["picks"]) == 130      # what every plain video looks like
    for edge in R.EVAL_EDGES:
        b = dict(base, n_steps=4000, picks=(15 * np.arange(4000)).astype(np.int32)) if edge == "pick_spacing_2" else base
        v = R.edge_video(b, edge)
        assert _EDGE_PRESENT[edge](v), edge
        assert (np.diff(v["picks"]) >= 0).all() and v["user_scores"].shape == v["user_summary"].shape == (3, v["n_frames"])
    seen = set()
    batch = R.eval_edge_batch()
    for name, v, s in batch:
        assert s.shape == (v["n_steps"],) and s.dtype == np.float32
        n_int = len(v["picks"]) - 1 + int(v["picks"][-1] != v["n_frames"])
        assert v["n_steps"] <= n_int <= min(v["n_steps"] + 1, 4096)
        seen |= {e for e in R.EVAL_EDGES if _EDGE_PRESENT[e](v)}
    assert seen == set(R.EVAL_EDGES)                                             # the batch holds every edge
    by = {name: (v, s) for name, v, s in batch}
    assert {v["user_summary"].shape[0] for _, v, _ in batch} == {1, 2, 31, 32}
    v, s = by["picks_from_15+zeros"]
    assert (s == 0).sum() >= 10 and v["picks"][0] == 15                          # intervals whose score ties with the uncovered frames' 0
    v, s = by["steps_4095+one_more_interval"]
    assert len(v["picks"]) == 4096 and v["picks"][-1] != v["n_frames"] and v["n_steps"] == 4095      # 4096 intervals: ED_MAX_INT exactly
    v, s = by["negative_scores"]
    assert (s < 0).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
    assert (by["all_zero+picks_from_7"][1] == 0).all()


@pytest.mark.parametrize("method", ["knapsack", "rank"])
def test_host_eval_tail_on_the_edge_batch_vs_numpy_oracle(method):
    """The native host tail (eval_native.evaluate_batch) on R.eval_edge_batch() against the literal oracle (eval_np: upsample,
    segment_scores, generate_summary, evaluate_summary, evaluate_scores = scipy rankdata + spearmanr): summaries and F-scores bit for
    bit, Spearman at test_host_eval.py's gate.  This pins the host tail as the reference tests/test_gpu_evaltail.py compares the device
    tail with.  One video is not the reference's to define: a change point that starts below 0 is a numpy slice that wraps round to
    the video's end (an empty slice here: mean NaN, then `int(nan)` raises ValueError in the reference's knapsack); the host and
    device tails clamp it to frame 0, and the oracle is given the clamped start."""
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    batch = R.eval_edge_batch()
    vids = [eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"],
                                      E.rank_users(v["user_scores"])) for _, v, _ in batch]
    corr, f_avg, f_max, summ = eval_native.evaluate_batch(vids, [s for _, _, s in batch], 0.15, method, want_summaries=True, n_threads=3)
    n_nan = 0
    for i, (name, v, s) in enumerate(batch):
        cps = v["change_points"].copy()
        if name == "cps_start_below_0":
            assert cps[0, 0] < 0
            cps[0, 0] = 0
        else:
            assert cps.min() >= 0
        s_ref = eval_np.generate_summary(s, cps, v["n_frames"], v["n_frame_per_seg"].tolist(), v["picks"], 0.15, method)
        np.testing.assert_array_equal(summ[i], s_ref, err_msg=name)
        fa, fm = eval_np.evaluate_summary(s_ref, v["user_summary"])
        assert float(fa) == f_avg[i] and float(fm) == f_max[i], (name, method, fa, f_avg[i], fm, f_max[i])
        with np.errstate(invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")                                      # scipy's ConstantInputWarning on the all-tied videos
            c_ref = eval_np.evaluate_scores(eval_np.upsample(s, v["n_frames"], v["picks"]), v["user_scores"])
        np.testing.assert_allclose(corr[i], c_ref, rtol=1e-12, atol=1e-14, equal_nan=True, err_msg=name)
        n_nan += int(np.isnan(c_ref))
    assert n_nan == 2                                                            # n_frames_1 and all_zero+picks_from_7, by construction


def test_host_eval_tail_refuses_scores_two_short_of_the_intervals():
    """lens two or more short of the interval count: the reference's loop raises IndexError (eval.py:29-34, scores[i] past the end),
    the oracle does the same, the host tail returns an error."""
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    v = R.synthetic_video(40, 8250, n_users=2)
    pv = eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"], E.rank_users(v["user_scores"]))
    s = np.linspace(0, 1, 38, dtype=np.float32)
    with pytest.raises(IndexError):
        eval_np.upsample(s, v["n_frames"], v["picks"])
    with pytest.raises(_lib.SumkError, match="more pick intervals than scores"):
        eval_native.evaluate_batch([pv], [s], 0.15, "knapsack")
    eval_native.evaluate_batch([pv], [np.linspace(0, 1, 39, dtype=np.float32)], 0.15, "knapsack")        # one short is the defined case


# ------------------------------------------------------------------------------------------------ DSN reward terms and REINFORCE loss
def test_reward_terms_is_what_compute_reward_returns():
    g = load_golden("reward")
    for ci in range(5):
        for far in (False, True):
            for dt in (np.float32, np.float64):
                d, r, rew = reward_np.reward_terms(g[f"c{ci}/seq"], g[f"c{ci}/actions"], far, 20, dt)
                got = reward_np.compute_reward(g[f"c{ci}/seq"], g[f"c{ci}/actions"], far_sim=far, dtype=dt)
                assert type(got) is dt and got.tobytes() == rew.tobytes()
                assert rew == dt((d + r) * dt(0.5)) and 0 <= r <= 1
    assert reward_np.reward_terms(g["c3/seq"], g["c3/actions"], False, 20, np.float64) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("family", R.REWARD_FAMILIES)
def test_reward_recipes_show_both_terms_in_fp32(family):
    """The conditions tests/test_gpu_reward_f64.py relies on, on the oracle alone: every reward it compares has 0.2 <= R_rep <= 1 (both
    terms are far above the gate of about 1e-6), the fp32 oracle -- the yardstick -- is within 1e-6 of the float64 one, and the cases
    that isolate a term do so in float64."""
    worst, n = 0.0, 0
    for call in R.reward_family(family):
        off = np.concatenate([[0], np.cumsum(call["lens"])])
        for e in range(call["acts"].shape[0]):
            for s, x in enumerate(call["xs"]):
                a = call["acts"][e, off[s]:off[s + 1]]
                d64, r64, rew64 = reward_np.reward_terms(x, a, call["far_sim"], call["thre"], np.float64)
                rew32 = reward_np.compute_reward(x, a, call["far_sim"], call["thre"], np.float32)
                what = call.get("expect", {}).get((e, s))
                cid = (call["id"], e, s, what)
                if what == "no_pick":
                    assert not np.nonzero(a)[0].size and rew64 == 0 and rew32 == 0, cid
                    continue
                assert np.nonzero(a)[0].size >= 1 and np.isfinite(rew64), cid
                assert 0.2 <= r64 <= 1 + 1e-12, (cid, r64)
                assert abs(float(rew32) - rew64) <= 1e-6, (cid, rew32, rew64)
                worst, n = max(worst, abs(float(rew32) - rew64)), n + 1
                if what == "one_pick":
                    assert d64 == 0 and rew64 == r64 / 2, cid
                elif what == "all_picked":
                    assert abs(r64 - 1) < 1e-12, (cid, r64)
                elif what == "beyond_thre":                          # two picks more than `thre` apart: R_div = 1 unless far_sim
                    assert (abs(d64 - 1) < 1e-12) != call["far_sim"], (cid, d64)
                elif what == "within_thre":                          # R_div = 1 - cos: the features are non-negative, so well below 1
                    assert 0 < d64 < 0.9, (cid, d64)
    print("REWARD-RECIPES", family, "cases", n, "largest |fp32 oracle - float64 oracle|", worst)
    assert n > 0


@pytest.mark.parametrize("beta", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("E", [1, 17])
def test_policy_np_vs_bernoulli_log_prob_autograd_in_float64(E, beta):
    """oracle/policy_np (forward and gradient, the closed clamp range included) against torch.distributions.Bernoulli.log_prob with
    autograd in float64.  The probabilities are clamped with finfo(float32).eps in front of the distribution (whose own float64 clamp
    is then idle): the kernels mirror the fp32 program."""
    from torch.distributions import Bernoulli
    from oracle import policy_np
    c = R.policy_case("short", E)
    lens, eps = c["lens"], 0.5
    off = np.concatenate([[0], np.cumsum(lens)])
    ce = float(np.finfo(np.float32).eps)
    assert policy_np.CLAMP == ce == float(R.POLICY_CLAMP)
    p = torch.from_numpy(c["probs"].astype(np.float64)).requires_grad_(True)
    a, r, b, w = (torch.from_numpy(c[k].astype(np.float64)) for k in ("actions", "rewards", "base", "dlv"))
    logp = Bernoulli(probs=p.clamp(ce, 1 - ce), validate_args=False).log_prob(a)                                   # (E, R)
    lv = torch.stack([beta * (p[off[v]:off[v + 1]].mean() - eps) ** 2 - (logp[:, off[v]:off[v + 1]].mean(dim=1) * (r[:, v] - b[v])).sum()
                      for v in range(len(lens))]) / E
    (lv * w).sum().backward()
    got_l, cond = policy_np.forward(c["probs"], lens, c["actions"], c["rewards"], c["base"], beta, eps, np.float64)
    got_g, mag = policy_np.backward(c["probs"], lens, c["actions"], c["rewards"], c["base"], beta, eps, c["dlv"], np.float64)
    np.testing.assert_allclose(got_l, lv.detach().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got_g, p.grad.numpy(), rtol=1e-11, atol=1e-300)
    assert (np.abs(got_g) <= mag * (1 + 1e-12)).all() and cond.min() >= 1 - 1e-12
    # outside the closed clamp range only the length penalty is left; ON its ends (eps, 1 - eps) the log-prob gradient passes
    out = c["outside"]
    assert out.size >= 5 and np.isin(np.flatnonzero((c["probs"] == R.POLICY_CLAMP) | (c["probs"] == 1 - R.POLICY_CLAMP)), out).sum() == 0
    vid = np.searchsorted(off, out, side="right") - 1
    mp = np.array([c["probs"][off[v]:off[v + 1]].astype(np.float64).mean() for v in range(len(lens))])
    want = c["dlv"].astype(np.float64)[vid] * 2 * beta * (mp[vid] - eps) / (E * np.asarray(lens)[vid])
    np.testing.assert_allclose(p.grad.numpy()[out], want, rtol=1e-12, atol=0)
    on_end = np.flatnonzero((c["probs"] == R.POLICY_CLAMP) | (c["probs"] == 1 - R.POLICY_CLAMP))
    live = on_end[c["dlv"][np.searchsorted(off, on_end, side="right") - 1] != 0]
    vl = np.searchsorted(off, live, side="right") - 1
    pen = c["dlv"].astype(np.float64)[vl] * 2 * beta * (mp[vl] - eps) / (E * np.asarray(lens)[vl])
    # (|sum_e adv_e (a - pc) / (pc (1 - pc))| >= 0.2 there: these videos' advantages have one sign and |a - pc| / (pc (1 - pc)) >= 1)
    assert live.size and (np.abs(p.grad.numpy()[live] - pen) >= 0.2 * np.abs(c["dlv"][vl]) / (E * np.asarray(lens)[vl])).all()
