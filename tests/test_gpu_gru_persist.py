"""The persistent GRU recurrence (csrc/gru_persist.hip: `DSN(cell="gru")`, H <= 256) against float64 nn.GRU
(oracle.torch_port.make_gru(dtype=float64)), forward and BPTT, at the model's size and over the shapes that sit on the
kernels' boundaries.  Gates, the ones the suite applies to its recurrent kernels (test_gpu_sumgan_full.py, test_gpu_gru.py):
  hidden states   max |d| <= 2e-5
  scores          max |d| <= 1e-4
  gradients       max |d| <= 3e-4 x max |ref|, per parameter tensor, and dx per video
Stock fp32 nn.GRU against the float64 one stays ~30x inside them on the full-size batch (h 7e-7, scores 8e-8, dx 9e-7, worst
parameter gradient 3.5e-6).  Device allocations are poisoned (all-ones bytes) in the full-size and the shape-walk cases: the
kernels may read no scratch they did not write."""
import functools

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence

import recipes as R
from oracle import torch_port
from test_gpu_sumgan_full import Gates, Poison

pytestmark = pytest.mark.gpu
F64 = torch.float64
H_GATE, S_GATE, G_GATE = 2e-5, 1e-4, 3e-4
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _health_is_clean():
    yield
    from summarizer_amd import kernels
    kernels.health_check()       # raises if any bounded hand-off wait timed out during the test


def full_lens(n=50):
    return [int(v) for v in np.ceil(np.random.default_rng(0).uniform(150, 320, 50))][:n]


def _layer_weights(sd, l):
    """The eight nn.GRU tensors of layer l in the C ABI's order: forward direction, then reverse."""
    return [sd[f"rnn.{n}_l{l}{suf}"] for suf in ("", "_reverse") for n in NAMES]


def _ref_stack(sd, xs, D, H, L, cw):
    """float64 reference: a stack of single-layer bidirectional nn.GRU (= nn.GRU(num_layers=L) without dropout), so that every
    layer's hidden states are at hand.  Returns per-layer h [(T_i, 2H)], scores, and the gradients of sum(scores * cw)."""
    grus = []
    for l in range(L):
        one = {k.replace(f"_l{l}", "_l0"): v for k, v in sd.items() if k.startswith("rnn.") and f"_l{l}" in k}
        grus.append(torch_port.make_gru(one, "rnn.", D if l == 0 else 2 * H, H, 1, dtype=F64))
    hw = sd["out.0.weight"].to(F64).requires_grad_(True)
    hb = sd["out.0.bias"].to(F64).requires_grad_(True)
    xr = [torch.from_numpy(x).to(F64).requires_grad_(True) for x in xs]
    seq, hs = xr, []
    for g in grus:
        out, lens = pad_packed_sequence(g(pack_sequence(seq, enforce_sorted=False))[0])
        seq = [out[:int(T), i] for i, T in enumerate(lens)]
        hs.append(seq)
    scores = [torch.sigmoid(torch.nn.functional.linear(h, hw, hb))[:, 0] for h in seq]
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])])
    loss = sum((s * cw[off[i]:off[i + 1]].to(F64)).sum() for i, s in enumerate(scores))
    loss.backward()
    grads = {"out.0.weight": hw.grad, "out.0.bias": hb.grad}
    for l, g in enumerate(grus):
        for k, v in g.named_parameters():
            grads["rnn." + k.replace("_l0", f"_l{l}")] = v.grad
    return dict(h=[[t.detach() for t in layer] for layer in hs], scores=[s.detach() for s in scores], grads=grads,
                dx=[t.grad for t in xr])


@functools.lru_cache(maxsize=None)
def full_case(D, H, L, n_videos=50):
    from summarizer_amd.models.dsn import DSN
    torch.manual_seed(1000 + H + L)
    sd = {k: v.detach().clone() for k, v in DSN(D, H, L, cell="gru").state_dict().items()}
    lens = full_lens(n_videos)
    xs = [(R.features(T, 1, D, 300 + i) - 0.2)[:, 0, :] for i, T in enumerate(lens)]
    cw = torch.from_numpy(np.random.default_rng(4).standard_normal(sum(lens)).astype(np.float32))
    return dict(D=D, H=H, L=L, sd=sd, lens=lens, xs=xs, cw=cw, ref=_ref_stack(sd, xs, D, H, L, cw))


def _model(case):
    from summarizer_amd.models.dsn import DSN
    m = DSN(case["D"], case["H"], case["L"], cell="gru")
    m.load_state_dict(case["sd"])
    return m.to(_dev())


def _train_once(case):
    """One scoring + backward through the model: (scores, {name: grad}, dx), all on the device."""
    m = _model(case)
    xp = torch.from_numpy(np.concatenate(case["xs"])).to(_dev()).requires_grad_(True)
    s = m.score_packed(xp, case["lens"])
    (s * case["cw"].to(_dev())).sum().backward()
    return s.detach(), {k: p.grad for k, p in m.named_parameters()}, xp.grad


def _gate_model(gt, case, s, grads, dx):
    ref, off = case["ref"], np.concatenate([[0], np.cumsum(case["lens"])])
    for i in range(len(case["lens"])):
        gt.fwd(f"scores[video {i}]", s[off[i]:off[i + 1]], ref["scores"][i], S_GATE)
        gt.grad(f"dx[video {i}]", dx[off[i]:off[i + 1]], ref["dx"][i], G_GATE)
    for k, g in grads.items():
        gt.grad(k, g, ref["grads"][k], G_GATE)


def _gate_hidden(gt, case, ws_exact=False):
    """Hidden states of every layer through the layer call of the C ABI, without grad (ws_exact: on a caller-owned workspace of
    exactly sumk_bigru_workspace_bytes(training = 0) bytes)."""
    from summarizer_amd import kernels
    dev = _dev()
    sb = kernels.SeqBatch.get(case["lens"], dev)
    off = np.concatenate([[0], np.cumsum(case["lens"])])
    sd = {k: v.to(dev) for k, v in case["sd"].items()}
    h = torch.from_numpy(np.concatenate(case["xs"])).to(dev)
    with torch.no_grad():
        for l in range(case["L"]):
            ws = None
            if ws_exact:
                nb = kernels.bigru_workspace_bytes(h.shape[1], case["H"], sb, training=False)
                assert nb < kernels.bigru_workspace_bytes(h.shape[1], case["H"], sb, training=True)
                ws = torch.empty(nb, dtype=torch.uint8, device=dev).fill_(255)
            h, kept = kernels.bigru_layer_forward(h, sb, _layer_weights(sd, l), case["H"], training=False, ws=ws)
            assert kept is None
            for i in range(len(case["lens"])):
                gt.fwd(f"h[layer {l}, video {i}]", h[off[i]:off[i + 1]], case["ref"]["h"][l][i], H_GATE)


# ------------------------------------------------------------------------------------------------ 1. full size through the model
@pytest.mark.parametrize("L", [1, 2])
def test_full_size_model_vs_float64(L, monkeypatch):
    case = full_case(1024, 256, L)
    gt = Gates(f"DSN gru D 1024 H 256 L {L}, 50 videos, poisoned")
    with Poison(monkeypatch):
        s, grads, dx = _train_once(case)
        _gate_model(gt, case, s, grads, dx)
        _gate_hidden(gt, case)
    gt.finish()


# ------------------------------------------------------------------------------------------------ 2. shape walk through the layer call
def _walk_lens(n, seed):
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(1, 24, n)]
    lens[0] = 1                                  # a one-frame video
    lens[n // 2] = 97                            # one video much longer than the rest (n = 1: the only one)
    if n > 2:
        lens[-1] = 1
    return lens


@pytest.mark.parametrize("In", [64, 1024])
@pytest.mark.parametrize("H", [4, 16, 40, 200, 252, 256])
def test_shape_walk_layer_call(H, In, monkeypatch):
    from summarizer_amd import kernels
    dev = _dev()
    gt = Gates(f"bigru layer H {H} In {In}")
    for n in (1, 13, 16, 17, 32, 33, 65):
        lens = _walk_lens(n, 7 * n + H)
        torch.manual_seed(H * 1000 + In + n)
        gru = torch.nn.GRU(In, H, bidirectional=True)
        sd = {"rnn." + k: v.detach().clone() for k, v in gru.state_dict().items()}
        ref_gru = torch_port.make_gru(sd, "rnn.", In, H, 1, dtype=F64)
        xs = [torch.from_numpy((R.features(T, 1, In, 40 + i) - 0.2)[:, 0, :]) for i, T in enumerate(lens)]
        cw = torch.from_numpy(np.random.default_rng(n).standard_normal((sum(lens), 2 * H)).astype(np.float32))
        off = np.concatenate([[0], np.cumsum(lens)])
        xr = [x.to(F64).requires_grad_(True) for x in xs]
        out, _ = pad_packed_sequence(ref_gru(pack_sequence(xr, enforce_sorted=False))[0])
        href = [out[:T, i] for i, T in enumerate(lens)]
        sum((h * cw[off[i]:off[i + 1]].to(F64)).sum() for i, h in enumerate(href)).backward()
        gref = {k: v.grad for k, v in ref_gru.named_parameters()}

        sb = kernels.SeqBatch.get(lens, dev)
        w = [sd[f"rnn.{nm}_l0{suf}"].to(dev) for suf in ("", "_reverse") for nm in NAMES]
        xp = torch.cat(xs).to(dev)
        with Poison(monkeypatch):
            h, ws = kernels.bigru_layer_forward(xp, sb, w, H, training=True)
            grads = [torch.zeros_like(t) for t in w]
            dx = kernels.bigru_layer_backward(xp, h, cw.to(dev), sb, w, grads, H, ws, want_dx=True)
        for i in range(n):
            gt.fwd(f"n {n} h[video {i}, T {lens[i]}]", h[off[i]:off[i + 1]], href[i].detach(), H_GATE)
            gt.grad(f"n {n} dx[video {i}, T {lens[i]}]", dx[off[i]:off[i + 1]], xr[i].grad, G_GATE)
        for d, suf in enumerate(("", "_reverse")):
            for j, nm in enumerate(NAMES):
                gt.grad(f"n {n} {nm}_l0{suf}", grads[4 * d + j], gref[f"{nm}_l0{suf}"], G_GATE)
    gt.finish()


# ------------------------------------------------------------------------------------------------ 3. the path is really taken
def _errors(case, s, grads, dx):
    ref, off = case["ref"], np.concatenate([[0], np.cumsum(case["lens"])])
    sc = max(float((s[off[i]:off[i + 1]].to(F64).cpu() - ref["scores"][i]).abs().max()) for i in range(len(case["lens"])))
    dxe = max(float((dx[off[i]:off[i + 1]].to(F64).cpu() - ref["dx"][i]).abs().max() / ref["dx"][i].abs().max()) for i in range(len(case["lens"])))
    ge = max(float((g.to(F64).cpu() - ref["grads"][k]).abs().max() / ref["grads"][k].abs().max()) for k, g in grads.items())
    return sc, dxe, ge


def test_persistent_path_is_taken_and_step_path_serves_larger_cells(monkeypatch):
    from summarizer_amd import kernels
    calls = {"n": 0}

    def forbid(name):
        def f(*a, **k):
            raise AssertionError(f"kernels.{name} called: the step path ran")
        return f

    def count(fn):
        def f(*a, **k):
            calls["n"] += 1
            return fn(*a, **k)
        return f

    real = {n: getattr(kernels, n) for n in ("gru_cell_forward", "gru_cell_backward", "linear_forward")}
    case = full_case(1024, 256, 1, 8)
    for n in real:
        monkeypatch.setattr(kernels, n, forbid(n))
    gt = Gates("H 256, step-path entry points raise")
    s, grads, dx = _train_once(case)                       # scores and trains without them
    _gate_model(gt, case, s, grads, dx)
    gt.finish()
    persist = _errors(case, s, grads, dx)

    for n in real:
        monkeypatch.setattr(kernels, n, count(real[n]))
    big = full_case(1024, 260, 1, 8)
    gt = Gates("H 260: step path")
    _gate_model(gt, big, *_train_once(big))
    gt.finish()
    assert calls["n"] > 3 * max(big["lens"]), calls        # it does call them, every step
    calls["n"] = 0
    _train_once(case)
    assert calls["n"] == 0                                  # and H = 256 never does

    monkeypatch.setattr(kernels, "bigru_eligible", lambda In, H: False)      # the step path at H = 256, against the same float64 reference
    gt = Gates("H 256 on the step path")
    s2, grads2, dx2 = _train_once(case)
    assert calls["n"] > 3 * max(case["lens"])
    _gate_model(gt, case, s2, grads2, dx2)
    gt.finish()
    step = _errors(case, s2, grads2, dx2)
    print("\nH 256 vs float64        scores      dx (rel)    worst parameter gradient (rel)")
    print(f"  persistent path      {persist[0]:.2e}    {persist[1]:.2e}    {persist[2]:.2e}")
    print(f"  step path            {step[0]:.2e}    {step[1]:.2e}    {step[2]:.2e}")


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_three_training_steps_are_bit_identical():
    case = full_case(1024, 256, 1)
    runs = [_train_once(case) for _ in range(3)]
    s0, g0, dx0 = runs[0]
    for s, g, dx in runs[1:]:
        assert torch.equal(s, s0) and torch.equal(dx, dx0)
        for k in g0:
            assert torch.equal(g[k], g0[k]), k


# ------------------------------------------------------------------------------------------------ 5. inference saves nothing
def test_inference_workspace_is_smaller_and_sufficient():
    case = full_case(1024, 256, 1)
    gt = Gates("no-grad forward on a workspace of exactly the inference size")
    _gate_hidden(gt, case, ws_exact=True)
    gt.finish()
    m = _model(case).eval()
    with torch.no_grad():
        s = m.score_packed(torch.from_numpy(np.concatenate(case["xs"])).to(_dev()), case["lens"])
    assert not s.requires_grad
    off = np.concatenate([[0], np.cumsum(case["lens"])])
    gt = Gates("no-grad scores")
    for i in range(len(case["lens"])):
        gt.fwd(f"scores[video {i}]", s[off[i]:off[i + 1]], case["ref"]["scores"][i], S_GATE)
    gt.finish()
