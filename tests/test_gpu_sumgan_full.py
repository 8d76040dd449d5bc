"""SumGAN's recurrent kernels at the sizes the model runs (the reference's defaults, what `bench.py --model sumgan` times)
against float64 CPU references (oracle/torch_port.py: lstm_stack_ref, dlstm_ref, make_gru(dtype=float64); pinned against
the real reference modules by tests/test_oracle.py).

Every case checks every forward output and the gradient of a fixed random-weighted scalar loss w.r.t. every parameter,
the input and the initial state, video by video and layer by layer (an error confined to one video or one partial tile
is not averaged away).  Gates, the ones the suite applies to the same kernels at small sizes:
  forward     max |d| <= 1e-4 on x_hat / mu / logvar / probabilities, <= 2e-5 on h / c states;
  gradients   max |d| <= 3e-4 x max |ref| of the same slice (fp32), 1e-3 (bf16x3).
The sizes reach the parts of the kernels (csrc/lstm.hip) that small sizes never run: the mat-vec forward's second k-chunk
(H > 1024), several 256-column strips and a partial one (H = 1060 = 4 x 256 + 36), many k-splits in lstm_cellbwd_kernel,
partial unit / column blocks, the many-sequence step kernels of the stack AND of the decoder (> 8 sequences) and a second
32-sequence m-tile that holds one video."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_port

pytestmark = pytest.mark.gpu
F64 = torch.float64
OUT_GATE, STATE_GATE = 1e-4, 2e-5
GRAD_GATE = {"fp32": 3e-4, "bf16x3": 1e-3}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _randn(shape, seed, scale=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _leaves(sd):
    return {k: v.detach().to(F64).requires_grad_(True) for k, v in sd.items()}


def _sub(p, prefix):
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


def _ref_grads(loss, named):
    names = list(named)
    return dict(zip(names, torch.autograd.grad(loss, [named[n] for n in names])))


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(int)


class Gates:
    """Collects every comparison of one case, prints the worst measured values, then fails listing everything over its gate
    (so one run reports all of a case's numbers)."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def fwd(self, what, got, ref, gate):
        d = float((got.detach().to(F64).cpu() - ref.detach()).abs().max())
        self.rows.append((what, "state" if gate == STATE_GATE else "out", d, gate))

    def grad(self, what, got, ref, gate):
        ref = ref.detach()
        scale = float(ref.abs().max())
        assert scale > 0, f"{self.case} {what}: reference gradient is zero"
        d = float((got.detach().to(F64).cpu() - ref).abs().max()) / scale
        self.rows.append((what, "grad", d, gate))

    def finish(self):
        worst = {}
        for what, kind, d, _ in self.rows:
            if not (d <= worst.get(kind, (-1.0, ""))[0]):
                worst[kind] = (d, what)
        print(f"\n[{self.case}] {len(self.rows)} checks; worst " +
              ", ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in sorted(worst.items())))
        bad = [f"{what}: {d:.3e} > {gate:.0e}" for what, _, d, gate in self.rows if not d <= gate]
        assert not bad, f"{self.case}: {len(bad)} of {len(self.rows)} over the gate: " + "; ".join(bad[:12])


class Poison:
    """Device allocations without initialisation come back as all-ones bytes (NaN as fp32), the pattern of
    tests/test_gpu_poison.py: a kernel that reads scratch nobody wrote then fails its gates."""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch

    def __enter__(self):
        from summarizer_amd import kernels
        empty, empty_like, ws = torch.empty, torch.empty_like, kernels.workspace

        def fill(t):
            if isinstance(t, torch.Tensor) and t.is_cuda and t.numel() and t.is_contiguous():
                t.reshape(-1).view(torch.uint8).fill_(255)
            return t
        self.mp.setattr(torch, "empty", lambda *a, **k: fill(empty(*a, **k)))
        self.mp.setattr(torch, "empty_like", lambda *a, **k: fill(empty_like(*a, **k)))
        self.mp.setattr(kernels, "workspace", lambda *a, **k: fill(ws(*a, **k)))
        return self

    def __exit__(self, *exc):
        self.mp.undo()
        return False


# ------------------------------------------------------------------------------------------------ eLSTM / cLSTM modules
def _module_case(kind, In, H, L, B, T, seed):
    """Weights, input, loss weights and the float64 reference of an eLSTM ("e") or cLSTM ("c") module."""
    from summarizer_amd.models.sumgan import eLSTM, cLSTM
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in (eLSTM if kind == "e" else cLSTM)(In, H, L).state_dict().items()}
    x = _randn((T, B, In), seed + 1, 0.5)
    p = _leaves(sd)
    xr = x.to(F64).requires_grad_(True)
    _, (hn, cn) = torch_port.lstm_stack_ref(list(xr.unbind(1)), _sub(p, "lstm."))
    if kind == "e":
        outs = {"h_mu": F.linear(hn, p["mu.weight"], p["mu.bias"]), "h_logvar": F.linear(hn, p["logvar.weight"], p["logvar.bias"]),
                "c_last": cn}
    else:
        outs = {"probs": torch.sigmoid(F.linear(hn[-1], p["out.0.weight"], p["out.0.bias"])), "h_last": hn[-1]}
    cw = {k: _randn(tuple(v.shape), seed + 10 + i) for i, (k, v) in enumerate(outs.items())}
    g = _ref_grads(sum((v * cw[k].to(F64)).sum() for k, v in outs.items()), {"x": xr, **p})
    return dict(kind=kind, sd=sd, x=x, cw=cw, ref={k: v.detach() for k, v in outs.items()}, g=g, L=L, B=B)


def _run_module(case, name, precision="fp32", grad=True):
    from summarizer_amd.models.sumgan import eLSTM, cLSTM
    dev = _dev()
    In, H = case["x"].shape[2], case["sd"]["lstm.weight_hh_l0"].shape[1]
    m = (eLSTM if case["kind"] == "e" else cLSTM)(In, H, case["L"])
    m.load_state_dict(case["sd"])
    for mod in m.modules():
        if hasattr(mod, "precision"):
            mod.precision = precision
    m = m.to(dev)
    x = case["x"].to(dev).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        r = m(x)
    outs = {"h_mu": r[0][0], "h_logvar": r[0][1], "c_last": r[1]} if case["kind"] == "e" else {"probs": r[0], "h_last": r[1]}
    gt = Gates(name)
    for k, v in outs.items():
        gate = STATE_GATE if k in ("c_last", "h_last") else OUT_GATE
        if v.dim() == 3:                      # (L, B, H)
            for l in range(v.shape[0]):
                for b in range(v.shape[1]):
                    gt.fwd(f"{k}[layer {l}, video {b}]", v[l, b], case["ref"][k][l, b], gate)
        else:                                 # (B, F)
            for b in range(v.shape[0]):
                gt.fwd(f"{k}[video {b}]", v[b], case["ref"][k][b], gate)
    if grad:
        sum((v * case["cw"][k].to(dev)).sum() for k, v in outs.items()).backward()
        gg = GRAD_GATE[precision]
        for b in range(x.shape[1]):
            gt.grad(f"dx[video {b}]", x.grad[:, b], case["g"]["x"][:, b], gg)
        for k, prm in m.named_parameters():
            gt.grad(f"d{k}", prm.grad, case["g"][k], gg)
    gt.finish()
    return {k: v.detach() for k, v in outs.items()}


@pytest.fixture(scope="module")
def s1():
    return _module_case("e", 1024, 2048, 2, 1, 300, 100)


@pytest.fixture(scope="module")
def s2():
    return _module_case("e", 1024, 2048, 2, 2, 300, 200)


@pytest.fixture(scope="module")
def s3():
    return _module_case("c", 1024, 1024, 2, 3, 300, 300)


def test_S1_elstm_bench_shape(s1):
    """eLSTM (In 1024, H 2048, L 2), one video of 300 frames, fp32: the mat-vec path with its second k-chunk, eight
    256-column strips of the transposed mat-vec and dh_last through lstm_cellbwd_kernel (mu / logvar read h_last).
    Measured on MI355X: mu / logvar 1.9e-7, c_last 3.2e-7, gradients 2.1e-6 of max |ref| (dx)."""
    _run_module(s1, "S1")


def test_S2_elstm_two_videos_bf16x3(s2):
    """eLSTM, the two score-weighted copies `SumGANTrainer._generate` feeds, bf16x3 input projections and dense layers.
    Measured: mu / logvar 1.0e-6, c_last 1.9e-6, gradients 1.4e-5 (dmu.weight)."""
    _run_module(s2, "S2", precision="bf16x3")


def test_S3_clstm(s3):
    """cLSTM (In 1024, H 1024, L 2): three videos of 300 frames, frame head on h_last.  Measured: probs 2.8e-8, h_last
    6.1e-8, gradients 2.5e-6 (dx)."""
    _run_module(s3, "S3")


# ------------------------------------------------------------------------------------------------ lstm_stack (ragged, h0 / c0)
def _stack_case(In, H, L, lens, with_state, seed):
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in torch.nn.LSTM(In, H, num_layers=L).state_dict().items()}
    B = len(lens)
    xs = [_randn((T, In), seed + 1 + i, 0.5) for i, T in enumerate(lens)]
    h0 = _randn((L, B, H), seed + 200, 0.3) if with_state else None
    c0 = _randn((L, B, H), seed + 201, 0.3) if with_state else None
    p = _leaves(sd)
    xr = [x.to(F64).requires_grad_(True) for x in xs]
    h0r = h0.to(F64).requires_grad_(True) if with_state else None
    c0r = c0.to(F64).requires_grad_(True) if with_state else None
    outs, (hn, cn) = torch_port.lstm_stack_ref(xr, p, h0r, c0r)
    cw_out = [_randn((T, H), seed + 300 + i) for i, T in enumerate(lens)]
    cw_h, cw_c = _randn((L, B, H), seed + 400), _randn((L, B, H), seed + 401)
    loss = sum((o * w.to(F64)).sum() for o, w in zip(outs, cw_out)) + (hn * cw_h.to(F64)).sum() + (cn * cw_c.to(F64)).sum()
    named = {**{f"x{i}": x for i, x in enumerate(xr)}, **p}
    if with_state:
        named.update(h0=h0r, c0=c0r)
    return dict(sd=sd, lens=lens, xs=xs, h0=h0, c0=c0, cw_out=cw_out, cw_h=cw_h, cw_c=cw_c, L=L, H=H,
                ref_out=[o.detach() for o in outs], ref_hn=hn.detach(), ref_cn=cn.detach(), g=_ref_grads(loss, named))


def _run_stack(case, name, grad=True):
    from summarizer_amd import kernels
    from summarizer_amd.models._bilstm import lstm_stack
    dev = _dev()
    lens, L, H = case["lens"], case["L"], case["H"]
    In = case["xs"][0].shape[1]
    lstm = torch.nn.LSTM(In, H, num_layers=L)
    lstm.load_state_dict(case["sd"])
    lstm = lstm.to(dev)
    if not grad:
        for prm in lstm.parameters():
            prm.requires_grad_(False)
    xp = torch.cat(case["xs"]).to(dev).requires_grad_(grad)
    h0 = None if case["h0"] is None else case["h0"].to(dev).requires_grad_(grad)
    c0 = None if case["c0"] is None else case["c0"].to(dev).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        out, hn, cn = lstm_stack(lstm, xp, kernels.SeqBatch.get(lens, dev), h0, c0)
    off = _offsets(lens)
    gt = Gates(name)
    for b in range(len(lens)):
        gt.fwd(f"out[video {b}, T={lens[b]}]", out[off[b]:off[b + 1]], case["ref_out"][b], STATE_GATE)
        for l in range(L):
            gt.fwd(f"h_n[layer {l}, video {b}]", hn[l, b], case["ref_hn"][l, b], STATE_GATE)
            gt.fwd(f"c_n[layer {l}, video {b}]", cn[l, b], case["ref_cn"][l, b], STATE_GATE)
    if grad:
        loss = (out * torch.cat(case["cw_out"]).to(dev)).sum() + (hn * case["cw_h"].to(dev)).sum() + (cn * case["cw_c"].to(dev)).sum()
        loss.backward()
        gg = GRAD_GATE["fp32"]
        for b in range(len(lens)):
            gt.grad(f"dx[video {b}, T={lens[b]}]", xp.grad[off[b]:off[b + 1]], case["g"][f"x{b}"], gg)
            if h0 is not None:
                for l in range(L):
                    gt.grad(f"dh0[layer {l}, video {b}]", h0.grad[l, b], case["g"]["h0"][l, b], gg)
                    gt.grad(f"dc0[layer {l}, video {b}]", c0.grad[l, b], case["g"]["c0"][l, b], gg)
        for k, prm in lstm.named_parameters():
            gt.grad(f"d{k}", prm.grad, case["g"][k], gg)
    gt.finish()
    return out.detach(), hn.detach(), cn.detach()


LENS_S4 = [100, 1, 37, 64, 5, 99, 12, 80, 2]                  # 9 videos: the first batch past the mat-vec path
LENS_S5_FEW = [60, 1, 33, 17, 40, 8, 59, 2]                   # 8 videos: still the mat-vec path
LENS_S5_MANY = [(7 * i) % 40 + 1 for i in range(33)]           # 33 videos: the second 32-sequence m-tile holds one


@pytest.fixture(scope="module")
def s4():
    return _stack_case(1024, 2048, 2, LENS_S4, True, 400)


@pytest.fixture(scope="module")
def s5_few():
    return _stack_case(1028, 1060, 2, LENS_S5_FEW, False, 500)


@pytest.fixture(scope="module")
def s5_many():
    return _stack_case(1028, 1060, 2, LENS_S5_MANY, True, 600)


def test_S4_stack_initial_state_nine_videos(s4):
    """lstm_stack (In 1024, H 2048, L 2) with h0 / c0 on 9 ragged videos (one of a single frame): lstm_step_kernel /
    lstm_bwd_step_kernel, loss on out, h_n and c_n.  Measured: states 4.8e-7, gradients 4.6e-6 (dx of the 80-frame video)."""
    _run_stack(s4, "S4")


def test_S5_stack_partial_tiles_mat_vec_path(s5_few):
    """In 1028, H 1060 = 4 x 256 + 36 (partial 256-column strip, partial unit block), 8 ragged videos: the mat-vec path.
    Measured: states 4.6e-7, gradients 1.8e-6."""
    _run_stack(s5_few, "S5 (8 videos)")


def test_S5_stack_partial_tiles_second_m_tile(s5_many):
    """In 1028, H 1060, 33 ragged videos with h0 / c0: partial 8-unit and 32-unit blocks, a second m-tile of one video.
    Measured: states 5.3e-7, gradients 2.6e-6 (dc0)."""
    _run_stack(s5_many, "S5 (33 videos)")


# ------------------------------------------------------------------------------------------------ inference == training
def test_I1_inference_equals_training(s1, s4):
    """Under torch.no_grad the stacks keep no per-row state and the last cell state comes from the running cstate, not
    from c_all: the outputs must pass the same float64 gates and equal the training-mode outputs (within 1e-6).  Measured:
    the no_grad outputs have the training-mode errors (S1 3.2e-7, S4 4.8e-7)."""
    for name, run in (("S1", lambda g: _run_module(s1, "I1/S1" + ("" if g else " no_grad"), grad=g)),
                      ("S4", lambda g: _run_stack(s4, "I1/S4" + ("" if g else " no_grad"), grad=g))):
        train, infer = run(True), run(False)
        items = zip(train.values(), infer.values()) if isinstance(train, dict) else zip(train, infer)
        for a, b in items:
            d = float((a - b).abs().max())
            assert d <= 1e-6, (name, d)


# ------------------------------------------------------------------------------------------------ dLSTM step-wise decoder
def _dec_case(H, L, D, lens, seed, module=True):
    """dLSTM weights (recons H -> D), h0 / c0, loss weights and the float64 reference.  module=False: no recons, the
    decoder kernels' raw top-layer rows (per-video lengths allowed)."""
    from summarizer_amd.models.sumgan import dLSTM
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in dLSTM(D, H, L).state_dict().items()}
    if not module:
        sd = {k: v for k, v in sd.items() if k.startswith("lstm.")}
    B = len(lens)
    h0, c0 = _randn((L, B, H), seed + 1, 0.4), _randn((L, B, H), seed + 2, 0.4)
    p = _leaves(sd)
    h0r, c0r = h0.to(F64).requires_grad_(True), c0.to(F64).requires_grad_(True)
    recons = (p["recons.weight"], p["recons.bias"]) if module else None
    ys = torch_port.dlstm_ref(_sub(p, "lstm."), recons, lens, h0r, c0r)
    cw = [_randn(tuple(y.shape), seed + 10 + i) for i, y in enumerate(ys)]
    g = _ref_grads(sum((y * w.to(F64)).sum() for y, w in zip(ys, cw)), {"h0": h0r, "c0": c0r, **p})
    return dict(sd=sd, lens=lens, h0=h0, c0=c0, cw=cw, ref=[y.detach() for y in ys], g=g, L=L, H=H, D=D)


def _dec_grads(gt, case, dh0, dc0, named_grads, gg):
    for l in range(case["L"]):
        for b in range(len(case["lens"])):
            gt.grad(f"dh0[layer {l}, video {b}]", dh0[l, b], case["g"]["h0"][l, b], gg)
            gt.grad(f"dc0[layer {l}, video {b}]", dc0[l, b], case["g"]["c0"][l, b], gg)
    for k, gr in named_grads:
        gt.grad(f"d{k}", gr, case["g"][k], gg)


def _run_dlstm(case, name, precision="fp32"):
    from summarizer_amd.models.sumgan import dLSTM
    dev = _dev()
    T, B = case["lens"][0], len(case["lens"])
    assert all(n == T for n in case["lens"])
    m = dLSTM(case["D"], case["H"], case["L"])
    m.load_state_dict(case["sd"])
    m.precision = precision
    m = m.to(dev)
    h0, c0 = case["h0"].to(dev).requires_grad_(True), case["c0"].to(dev).requires_grad_(True)
    x_hat = m(T, h0, c0)
    assert tuple(x_hat.shape) == (T, B, case["D"])
    gt = Gates(name)
    for b in range(B):
        gt.fwd(f"x_hat[video {b}]", x_hat[:, b], case["ref"][b], OUT_GATE)
    (x_hat * torch.stack(case["cw"], dim=1).to(dev)).sum().backward()
    _dec_grads(gt, case, h0.grad, c0.grad, [(k, prm.grad) for k, prm in m.named_parameters()], GRAD_GATE[precision])
    gt.finish()


@pytest.fixture(scope="module")
def d1():
    return _dec_case(2048, 2, 1024, [300], 700)


@pytest.fixture(scope="module")
def d2():
    return _dec_case(2048, 2, 1024, [160, 160], 800)


@pytest.fixture(scope="module")
def d3_wide():
    return _dec_case(2048, 2, 1024, [64] * 9, 900)


@pytest.fixture(scope="module")
def d3_deep():
    return _dec_case(1060, 3, 256, [40] * 33, 1000)


def test_D1_dlstm_bench_shape(d1):
    """dLSTM (H 2048, L 2, recons 2048 -> 1024), one video of 300 steps, fp32: the decoder's mat-vec path.  Measured:
    x_hat 2.7e-7, gradients 1.1e-6."""
    _run_dlstm(d1, "D1")


def test_D2_dlstm_two_videos_bf16x3(d2):
    """dLSTM on two videos of 160 steps (the trainer's batched passes), recons in bf16x3.  Measured: x_hat 1.1e-6,
    gradients 7.5e-6 (drecons.weight)."""
    _run_dlstm(d2, "D2", precision="bf16x3")


def test_D3_dlstm_many_sequences_h2048(d3_wide):
    """9 sequences: lstm_dec_step_kernel / lstm_dec_bwd_step_kernel at H 2048, L 2, 64 steps.  Measured: x_hat 3.9e-7,
    gradients 1.7e-6."""
    _run_dlstm(d3_wide, "D3 (H 2048, 9 videos)")


def test_D3_dlstm_many_sequences_h1060_three_layers(d3_deep):
    """33 sequences (second m-tile of one), H 1060 (partial unit / column blocks), L 3 (a middle layer), 40 steps.
    Measured: x_hat 2.8e-7, gradients 1.1e-6."""
    _run_dlstm(d3_deep, "D3 (H 1060, L 3, 33 videos)")


@pytest.fixture(scope="module")
def d4():
    return [_dec_case(1060, 1, 256, [50] * B, 1100 + B) for B in (1, 9)]


def test_D4_dlstm_single_layer(d4):
    """L = 1: the top layer is also layer 0, its output feeds its own next step through W_ih -- both paths, H 1060, 50
    steps.  Measured: x_hat 2.5e-7, gradients 6.7e-7."""
    for case in d4:
        _run_dlstm(case, f"D4 (L 1, {len(case['lens'])} videos)")


# ------------------------------------------------------------------------------------------------ ragged decoder (C ABI)
def _run_decoder_kernels(case, name):
    """kernels.lstm_decoder_forward / _backward directly, per-video lengths (dLSTM never makes them; the ABI accepts them)."""
    from summarizer_amd import kernels
    dev = _dev()
    lens, L, H = case["lens"], case["L"], case["H"]
    sb = kernels.SeqBatch.get(lens, dev)
    w = {k: v.to(dev) for k, v in case["sd"].items()}
    names = [[f"lstm.{n}_l{l}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] for l in range(L)]
    layers = [tuple(w[n] for n in ns) for ns in names]
    grads = [tuple(torch.zeros_like(w[n]) for n in ns) for ns in names]
    h0, c0 = case["h0"].to(dev).contiguous(), case["c0"].to(dev).contiguous()
    out, ws = kernels.lstm_decoder_forward(sb, layers, H, h0, c0)
    off = _offsets(lens)
    gt = Gates(name)
    for b in range(len(lens)):
        gt.fwd(f"out[video {b}, T={lens[b]}]", out[off[b]:off[b + 1]], case["ref"][b], STATE_GATE)
    dh0, dc0 = kernels.lstm_decoder_backward(sb, layers, H, c0, out, torch.cat(case["cw"]).to(dev), grads, ws, True)
    _dec_grads(gt, case, dh0, dc0, [(n, g) for ns, gs in zip(names, grads) for n, g in zip(ns, gs)], GRAD_GATE["fp32"])
    gt.finish()


@pytest.fixture(scope="module")
def d5():
    return [_dec_case(1060, 2, 16, lens, 1200 + len(lens), module=False)
            for lens in ([30, 1, 17, 29], [1, 25, 3, 40, 12, 7, 33, 2, 18, 9])]


def test_D5_decoder_ragged_lengths(d5):
    """Ragged decoder lengths through the C ABI, H 1060, 4 videos (mat-vec path) and 10 (many-sequence path), T = 1 in
    both: every video is decoded over its own steps only (the ABI computes ragged batches correctly).  Measured: outputs
    9.4e-8, gradients 6.5e-7."""
    for case in d5:
        _run_decoder_kernels(case, f"D5 ({len(case['lens'])} videos)")


# ------------------------------------------------------------------------------------------------ poisoned scratch
def test_poisoned_scratch_many_sequence_stack_and_decoder(monkeypatch, s4, d3_deep):
    """S4 and the 33-sequence decoder with every torch.empty / kernels.workspace allocation filled with 0xFF bytes (NaN):
    a read of scratch nobody wrote (e.g. dcstate at a video's last step) fails the float64 gates.  Measured: the same errors
    as the clean runs."""
    with Poison(monkeypatch):
        _run_stack(s4, "poisoned S4")
        _run_dlstm(d3_deep, "poisoned D3 (H 1060, L 3, 33 videos)")


# ------------------------------------------------------------------------------------------------ DSN(cell="gru")
LENS_G1 = [1, 40, 7, 100, 23, 2, 64, 15, 31, 9]


def _gru_case(L, lens, seed):
    from summarizer_amd.models.dsn import DSN
    D, H = 1024, 256
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in DSN(D, H, L, cell="gru").state_dict().items()}
    xs = [_randn((T, D), seed + 1 + i, 0.5).abs() for i, T in enumerate(lens)]
    p = _leaves(sd)
    gru = torch_port.make_gru(sd, "rnn.", D, H, L, dtype=F64)
    xr = [x.to(F64).requires_grad_(True) for x in xs]
    ys = [torch_port.bigru_scores(x.unsqueeze(1), p, "rnn.", "out.0.weight", "out.0.bias", gru)[:, 0, 0] for x in xr]
    cw = [_randn((T,), seed + 100 + i) for i, T in enumerate(lens)]
    named = {**{f"x{i}": x for i, x in enumerate(xr)}, **{f"rnn.{k}": v for k, v in gru.named_parameters()},
             "out.0.weight": p["out.0.weight"], "out.0.bias": p["out.0.bias"]}
    g = _ref_grads(sum((y * w.to(F64)).sum() for y, w in zip(ys, cw)), named)
    return dict(sd=sd, L=L, lens=lens, xs=xs, cw=cw, ref=[y.detach() for y in ys], g=g)


@pytest.fixture(scope="module", params=[(1, "single"), (1, "ragged"), (2, "single"), (2, "ragged")],
                ids=["L1-T300", "L1-ragged", "L2-T300", "L2-ragged"])
def g1(request):
    L, kind = request.param
    return _gru_case(L, [300] if kind == "single" else LENS_G1, 1300 + 10 * L + (kind == "ragged"))


def test_G1_dsn_gru(g1):
    """DSN(cell="gru") (D 1024, H 256): one video of 300 frames through forward(), and 10 ragged videos (one of a single
    frame) through score_packed; probabilities and every gradient.  Measured: probabilities 1.1e-7, gradients 2.1e-6."""
    from summarizer_amd.models.dsn import DSN
    dev = _dev()
    lens = g1["lens"]
    m = DSN(1024, 256, g1["L"], cell="gru")
    m.load_state_dict(g1["sd"])
    m = m.to(dev)
    xp = torch.cat(g1["xs"]).to(dev).requires_grad_(True)
    s = m(xp.unsqueeze(1))[:, 0, 0] if len(lens) == 1 else m.score_packed(xp, lens)
    off = _offsets(lens)
    gt = Gates(f"G1 (L {g1['L']}, {len(lens)} videos)")
    for b in range(len(lens)):
        gt.fwd(f"probs[video {b}, T={lens[b]}]", s[off[b]:off[b + 1]], g1["ref"][b], OUT_GATE)
    (s * torch.cat(g1["cw"]).to(dev)).sum().backward()
    gg = GRAD_GATE["fp32"]
    for b in range(len(lens)):
        gt.grad(f"dx[video {b}, T={lens[b]}]", xp.grad[off[b]:off[b + 1]], g1["g"][f"x{b}"], gg)
    for k, prm in m.named_parameters():
        gt.grad(f"d{k}", prm.grad, g1["g"][k], gg)
    gt.finish()
