"""GPU: the bidirectional LSTM recurrences of csrc/lstm.hip -- every forward form and every BPTT form that the layer's path plan can
give a shape (lstm_carve records the persistent form each pass is eligible for, LstmWs::fwd / bwd; lstm_usable applies the run-time
gates, and without a persistent form a few videos take the mat-vec BPTT, more the launch chain) -- against float64, video by video and
gate block by gate block.

tests/test_gpu_lstm.py and tests/test_gpu_train_full.py compare one kernel form with another (an error both share passes), scores within
1e-4 and whole-tensor gradient norms within 3e-4 (an error confined to one video, one 16/32-row tile, one gate block or one member's
units is averaged away).  Here the reference is oracle/torch_port.bilstm_stack_ref in float64 (pinned against nn.LSTM by
tests/test_oracle.py) and the yardstick is the SAME oracle in fp32 with the kernels' gate formulas (gate_math="rcp_form":
1 / (1 + exp(-v)), 1 - 2 / (1 + exp(2 v)), csrc/persist_common.h), as in tests/test_gpu_reward_f64.py:

  quantity   hidden states of every layer (kernels.bilstm_layer_forward, inference and training mode) per video and direction, scores
             (score_packed, inference and training mode) per video: largest absolute error of the slice;
             gradients of sum(scores * cw), cw fixed random: dx per video, every LSTM parameter per direction and per gate block
             (i, f, g, o: the four row quarters), the head's weight and bias: largest absolute error of the slice / largest reference
             magnitude of the slice.
  gate       HIP error <= 4 x yardstick.  Yardstick of a KIND (hidden states of a layer, scores, dx, weight_ih blocks, weight_hh
             blocks, bias blocks, head) = the largest |fp32 oracle - float64| over the case's slices of that kind (one slice can land
             on the float64 value by chance), with a floor of 2 fp32 ulps (2^-23) of the slice's largest reference magnitude.
  bf16x6     is advertised as fp32-grade: the plain fp32 yardstick.  TRAINING in bf16x6 keeps the exact-fp32 recurrence (the BPTT
             multiplies in fp32), so bf16x6 runs here are inference runs.
  bf16x3     a documented difference in arithmetic: the yardstick oracle makes the same roundings (torch_port.Linear3: hi.hi + hi.lo +
             lo.hi on two-plane operands) in exactly the products the library runs in that mode -- the input projections with their
             backward GEMMs (dx, dW_ih), and for H > 256 the recurrent product and dW_hh (the BPTT's dG . W_hh stays fp32).
The 4 x margin is the project's; a CPU emulation (2 ulp of noise on every exp, 1 ulp on every reciprocal: v_exp_f32 / v_rcp_f32 as
documented) put the hidden states at 1.7-2.3 x the yardstick at T = 90 ... 300.

Every case runs with uninitialised device allocations poisoned (Poison of tests/test_gpu_sumgan_full.py) and is followed by
kernels.health_check().  Each video has its own feature seed; every batch of more than three videos holds a one-frame video, a two-frame
video and ties in length.  References are cached per (case, arithmetic): forms and precisions share one CPU run.

Cases (H, D, videos; what the plan gives them):
  a  256, 128,   9 (<= 64 frames)  groups of 3: forward and BPTT on 16-row MFMAs, coalesced BPTT exchange (8 aligned units per member)
  b  256, 128,  70 (<= 40)         groups of 18: 32-row MFMAs, the last group partial
  c  256, 128, 140 (<= 24)         groups of 32, 10 work items on 8 teams (a team runs a second item); >= 1024 rows: in bf16x6 / bf16x3
                                   inference the projection runs on operand planes (In = 128, 8H % 256 == 0)
  d   40, 128,  34                 two units per member, a k tail, H not a multiple of 8
  e  100,  64,  20 (<= 30), L = 2  four units per member, 25 active members, uncoalesced BPTT exchange; layer 1 has In = 2H
  f 1024, 128,  43 (<= 70)         lstm_wide2_kernel, packed publish, tile boundary at 32 / 33 sorted rows; lstm_wide_bwd_kernel;
                                   fp32 and bf16x3 forward + backward, bf16x6 inference
  g  320,  64,  70 (<= 40)         two work items per direction, three units per member, scalar publish; BPTT: lstm_bwd_step_kernel
  h  384,  64,  77 (<= 40)         lstm_wide_bwd_kernel with two column groups
  i 1024,  64,   3 (<= 40)         BPTT on lstm_tgemv_partial_kernel / lstm_cellbwd_kernel, both directions (n <= 8); three videos
                                   leave no room for a tie: 40, 1 and 2 frames
  j 1028,  64,  10 (<= 12)         H > 1024: lstm_step_kernel and lstm_bwd_step_kernel
  k  256,  64,   1 of 1000 frames  forward only: error growth over a long chain of hand-offs
  l  case d in a child process with SUMK_LSTM_PERSIST=0: the launch-per-step kernels at H <= 256 ("same arithmetic")
  m  384,  64, 3969 (<= 3)         one video past what lstm_wide2_kernel's sharded counters hold (62 groups of 64): lstm_step_kernel at a
                                   wide H, inference; in training mode its saves feed lstm_wide_bwd_kernel (63 groups, one counter word
                                   per item) -- training-mode scores of every video, dx of the first and the last 64 videos

The dX GEMM of the backward (dx = dG_fwd W_ih_fwd + dG_rev W_ih_rev) sums its K = 4H gate columns per direction in ONE fp32 MFMA accumulator
(csrc/gemm_regstage.h); a BLAS product sums in blocks and lanes and its error grows far slower with K.  With a BLAS product in the yardstick
dx measured 0.9 x (H = 40), 2.5-3.1 x (H = 256) and 4.85 x (H = 1024: over the gate) while every other kind stayed below 1.5 x: the square
root of K, not a kernel error.  The fp32 yardstick therefore takes that one product as the kernel does (torch_port.LinearChainDx / mm_chain).

Figures, measured on MI355X (worst HIP error / yardstick per kind, 4 is the limit; the same with SUMK_TEST_POISON=1):
  case          hidden  scores    dx  weight_ih  weight_hh  bias  head     yardsticks: hidden / scores / dx
  a fp32          1.33    1.18  1.81       0.97       1.13  0.90  0.74     1.2e-7 / 6.5e-8 / 5.2e-7
  b fp32          1.07    0.96  1.26       0.85       1.09  1.26  0.45     1.4e-7 / 7.4e-8 / 1.0e-6
  c fp32          1.03    1.05  2.03       1.12       1.27  0.75  0.65     1.5e-7 / 7.6e-8 / 8.9e-7
  c bf16x6        0.96    0.96                                             (inference; the fp32 yardsticks)
  c bf16x3        1.00    1.00                                             1.1e-6 / 2.9e-7 (inference)
  d fp32          0.98    1.17  1.23       0.59       0.85  1.15  0.68     1.7e-7 / 7.4e-8 / 4.4e-7
  e fp32 (L 2)    1.21    1.00  1.10       1.18       1.29  1.44  1.13     1.1e-7 / 6.8e-8 / 5.3e-7
  f fp32          1.09    1.04  1.50       1.02       0.91  0.73  0.71     1.1e-7 / 7.5e-8 / 1.9e-6
  f bf16x3        1.02    1.05  0.98       1.19       0.99  1.04  0.84     5.8e-7 / 1.6e-7 / 6.7e-6
  f bf16x6        1.12    1.25                                             (inference; the fp32 yardsticks)
  g fp32          1.06    1.01  1.36       0.87       1.35  0.94  1.45     1.1e-7 / 7.0e-8 / 1.3e-6
  h fp32          1.14    1.00  1.27       1.08       0.88  0.65  1.70     1.2e-7 / 8.1e-8 / 1.4e-6
  i fp32          1.12    0.85  1.16       0.77       0.92  0.52  0.96     9.6e-8 / 6.5e-8 / 1.4e-6
  j fp32          0.26    0.74  1.20       0.50       0.40  0.48  0.19     9.4e-8 / 7.0e-8 / 1.3e-6
  k fp32          1.10    1.00                                             1.2e-7 / 7.3e-8 (forward only)
  l (d, steps)    0.84    0.73  1.23       0.44       0.57  1.25  0.33     (case d's)
  m fp32          0.44    0.71                                             1.1e-7 / 8.6e-8 (inference)
  m fp32 training         0.71  1.32                                       8.6e-8 / 1.3e-6 (scores / dx; dx of 128 videos)
  Parameter-gradient yardsticks lie between 3.8e-7 and 2.4e-6 (fp32) and 4.4e-6 and 8.1e-6 (bf16x3).  No kernel exceeded the gate.

What these gates see and the earlier ones (scores 1e-4, hidden states 2e-5, whole-tensor relative L2 3e-4) do not, shown on the CPU with the
fp32 oracle of case c standing in for the kernels (scripts/probes/lstm_f64_sensitivity.py):
  one video's rows of h, scores and dx off by 1e-6: slices at 7 x (hidden), 13 x (scores), 54 x (dx); whole-tensor L2 <= 1.7e-5;
  the last k chunk (8 of 256) of h . W_hh dropped for one unit of one video: 2500 x (hidden), 83 x (scores), 16000 x (its weight_hh block);
  scores move by 6.4e-6, the worst whole-tensor L2 is 6.1e-5;
  a two-frame video reading its neighbour's state in its last step: 1.8e5 x (hidden), 405 x (scores); scores move by 3.1e-5 (L2 1.5e-6), so
  an inference test passes -- the whole-tensor gradient norms DO see this one at 1720 rows (weight_hh 1.8e-2: one row's term in a sum of
  1720, about 1 / sqrt(rows)).
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recipes as R
from oracle import torch_port
from test_gpu_sumgan_full import Poison

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -24
FACTOR = 4.0
F64 = torch.float64
REPORT = []

CASES = {
    "a": dict(H=256, D=128, L=1, lens=[64, 1, 2, 33, 64, 17, 33, 40, 5]),
    "b": dict(H=256, D=128, L=1, lens=[40, 1, 2] + [(7 * i) % 40 + 1 for i in range(67)]),
    "c": dict(H=256, D=128, L=1, lens=[24, 1, 2] + [(5 * i) % 24 + 1 for i in range(137)]),
    "d": dict(H=40, D=128, L=1, lens=[50, 1, 33, 7, 2] + [4] * 29),
    "e": dict(H=100, D=64, L=2, lens=[30, 1, 2, 17, 30, 9, 25, 4, 12, 17, 3, 28, 7, 21, 5, 14, 1, 19, 8, 26]),
    "f": dict(H=1024, D=128, L=1, lens=[70, 33, 1, 70, 12] * 8 + [2, 64, 64]),
    "g": dict(H=320, D=64, L=1, lens=[40, 1, 2, 33] + [3, 7, 18] * 22),
    "h": dict(H=384, D=64, L=1, lens=[20, 7, 33, 12, 5, 40, 2, 18, 25, 9, 1] * 7),
    "i": dict(H=1024, D=64, L=1, lens=[40, 1, 2]),
    "j": dict(H=1028, D=64, L=1, lens=[12, 1, 2, 7, 12, 5, 9, 3, 7, 11]),
    "k": dict(H=256, D=64, L=1, lens=[1000], forward_only=True),
    "m": dict(H=384, D=64, L=1, lens=[3, 1, 2] + [(i % 3) + 1 for i in range(3966)], forward_only=True),
}
M_DX_VIDEOS = tuple(range(64)) + tuple(range(3969 - 64, 3969))     # case m in training mode: the videos whose dx is judged
SEED = {c: 4100 + 100 * i for i, c in enumerate(sorted(CASES))}
LSTM_TENSORS = (("weight_ih", "dweight_ih"), ("weight_hh", "dweight_hh"), ("bias_ih", "dbias"), ("bias_hh", "dbias"))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for r in REPORT:
        print("LSTM-F64-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "lstm_f64.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


@pytest.fixture(autouse=True)
def _health():
    yield
    from summarizer_amd import kernels
    kernels.health_check()


# ------------------------------------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Weights (recipes.lstm_weights), one feature block per video (its own seed) and the fixed loss weights of a case."""
    c = CASES[case]
    lens, seed = c["lens"], SEED[case]
    if len(lens) > 3:
        assert 1 in lens and 2 in lens and len(set(lens)) < len(lens), case
    assert max(lens) <= {"a": 64, "b": 40, "c": 24, "d": 50, "e": 30, "f": 70, "g": 40, "h": 40, "i": 40, "j": 12, "k": 1000, "m": 3}[case]
    w = R.lstm_weights("rnn.", c["D"], c["H"], c["L"], seed, "out.0.")
    xs = [R.features(T, 1, c["D"], seed + 1 + i)[:, 0, :] - 0.2 for i, T in enumerate(lens)]
    cw = np.random.default_rng(seed + 99).standard_normal(sum(lens)).astype(np.float32)
    return dict(w=w, xs=xs, cw=cw, off=np.concatenate([[0], np.cumsum(lens)]).astype(int))


@functools.lru_cache(maxsize=None)
def _oracle(case, mode, grads, videos=None):
    """bilstm_stack_ref + head + the gradients of sum(scores * cw).  mode "f64": float64, exact gate functions (the reference);
    "fp32": float32 with the kernels' gate formulas (the yardstick); "x3": the fp32 yardstick with the bf16x3 products where the
    library runs them.  videos: a tuple of video indices -- the batch of those videos alone, with their rows of cw (scores and dx of a
    video depend on that video alone).  Returns {name: float64 array}: h<l> (R, 2H), scores (R,), dx (R, D), the state_dict names.
    Never modified."""
    c, inp = CASES[case], _inputs(case)
    dt = F64 if mode == "f64" else torch.float32
    p = {k: torch.from_numpy(v).to(dt).requires_grad_(grads) for k, v in inp["w"].items()}
    vids = range(len(inp["xs"])) if videos is None else videos
    xs = [torch.from_numpy(inp["xs"][v]).to(dt).requires_grad_(grads) for v in vids]
    cw = np.concatenate([inp["cw"][inp["off"][v]:inp["off"][v + 1]] for v in vids])
    hook = None
    if mode == "fp32" and grads:     # the dX GEMM's one accumulator chain over 4H columns per direction (torch_port.mm_chain says why)
        hook = lambda a, w, site: torch_port.LinearChainDx.apply(a, w) if site == "ih" else a @ w.t()
    if mode == "x3":
        wide = c["H"] > 256          # sumk_bilstm_layer_forward: the wide kernels take the recurrent product in the layer's arithmetic
        hook = lambda a, w, site: (torch_port.Linear3.apply(a, w, site == "hh") if site == "ih" or wide else a @ w.t())
    sig = torch_port.GATE_MATH["exact" if mode == "f64" else "rcp_form"][0]
    with torch.set_grad_enabled(grads):
        layers = torch_port.bilstm_stack_ref(xs, {k[4:]: v for k, v in p.items() if k.startswith("rnn.")},
                                             gate_math="exact" if mode == "f64" else "rcp_form", matmul=hook)
        scores = sig(torch.cat(layers[-1]) @ p["out.0.weight"].t() + p["out.0.bias"])[:, 0]
        out = {f"h{l}": torch.cat(v) for l, v in enumerate(layers)}
        out["scores"] = scores
        if grads:
            names = list(p)
            g = torch.autograd.grad((scores * torch.from_numpy(cw).to(dt)).sum(), xs + [p[n] for n in names])
            out["dx"] = torch.cat(g[:len(xs)])
            out.update(zip(names, g[len(xs):]))
    return {k: v.detach().to(F64).numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the HIP side
def _hip(case, precision, grads, monkeypatch):
    """Hidden states of every layer through kernels.bilstm_layer_forward (as models._bilstm.bilstm_scores runs the layers), scores
    through DSN.score_packed; with grads also both in training mode and every gradient.  {name: float64 array}."""
    from summarizer_amd import kernels
    from summarizer_amd.models import _bilstm
    from summarizer_amd.models.dsn import DSN
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    c, inp = CASES[case], _inputs(case)
    H, D, L, lens = c["H"], c["D"], c["L"], c["lens"]
    m = DSN(D, H, L)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in inp["w"].items()})
    m.precision = precision
    m = m.to(dev)
    x = torch.from_numpy(np.concatenate(inp["xs"])).to(dev)
    out = {}
    with Poison(monkeypatch):
        sb = kernels.SeqBatch.get(lens, dev)
        p = dict(m.named_parameters())
        with torch.no_grad():
            wpl = _bilstm._layer_wplanes(m, p, "rnn.", L, D, H, precision) if sb.n_rows >= 1024 else None
            h = x
            for l in range(L):
                h, _ = kernels.bilstm_layer_forward(h, sb, p, "rnn.", l, H, training=False, precision=precision,
                                                    wplanes=None if wpl is None else wpl[l], dataset_input=(l == 0))
                out[f"h{l}"] = h
            out["scores"] = m.score_packed(x, lens)
            if grads:
                h = x
                for l in range(L):
                    h, _ = kernels.bilstm_layer_forward(h, sb, p, "rnn.", l, H, training=True, precision=precision)
                    out[f"train_h{l}"] = h
        if grads:
            xg = x.clone().requires_grad_(True)
            s = m.score_packed(xg, lens)
            (s * torch.from_numpy(inp["cw"]).to(dev)).sum().backward()
            out["train_scores"], out["dx"] = s.detach(), xg.grad
            out.update({k: prm.grad for k, prm in m.named_parameters()})
        out = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in out.items()}
    return out


# ------------------------------------------------------------------------------------------------ slices and the gate
def _slices(case, grads):
    """[(kind, name, key in the HIP dict, key in the oracle dicts, index, relative)] of a case."""
    c, off = CASES[case], _inputs(case)["off"]
    H, lens = c["H"], c["lens"]
    rows = lambda v: slice(off[v], off[v + 1])
    sl = []
    for mode in ("", "train_") if grads else ("",):
        for l in range(c["L"]):
            for v in range(len(lens)):
                for d, dn in enumerate(("fwd", "rev")):
                    sl.append((f"hidden_l{l}", f"{mode}h{l}[video {v}, T={lens[v]}, {dn}]", f"{mode}h{l}", f"h{l}",
                               (rows(v), slice(d * H, (d + 1) * H)), False))
        for v in range(len(lens)):
            sl.append(("scores", f"{mode}scores[video {v}, T={lens[v]}]", f"{mode}scores", "scores", (rows(v),), False))
    if grads:
        for v in range(len(lens)):
            sl.append(("dx", f"dx[video {v}, T={lens[v]}]", "dx", "dx", (rows(v),), True))
        for l in range(c["L"]):
            for suf in ("", "_reverse"):
                for t, kind in LSTM_TENSORS:
                    for q, gate in enumerate("ifgo"):
                        k = f"rnn.{t}_l{l}{suf}"
                        sl.append((kind, f"d{k}[{gate}]", k, k, (slice(q * H, (q + 1) * H),), True))
        for k in ("out.0.weight", "out.0.bias"):
            sl.append(("dhead", f"d{k}", k, k, (Ellipsis,), True))
    return sl


def _judge(tag, case, got, ref, yard, grads, slices=None):
    """Every slice of the case (or the given ones) against float64; prints and records yardsticks and worst ratios; fails listing what is
    over the gate."""
    rows, ys = [], {}
    for kind, name, gk, rk, idx, rel in (_slices(case, grads) if slices is None else slices):
        r = ref[rk][idx]
        scale = float(np.abs(r).max())
        assert scale > 0 and got[gk].shape == ref[rk].shape, (tag, name, scale, got[gk].shape, ref[rk].shape)
        den = scale if rel else 1.0
        ey = float(np.abs(yard[rk][idx] - r).max()) / den
        eh = float(np.abs(got[gk][idx] - r).max()) / den                  # NaN / inf: fails `eh <= gate` below
        rows.append((kind, name, eh, 2 * ULP * (1.0 if rel else scale)))
        ys[kind] = max(ys.get(kind, 0.0), ey)
    worst, bad = {}, []
    for kind, name, eh, floor in rows:
        y = max(ys[kind], floor)
        ratio = eh / y
        if not ratio <= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (ratio, name)
        if not eh <= FACTOR * y:
            bad.append(f"{name}: {eh:.3e} > {FACTOR:g} x {y:.3e}")
    REPORT.append(dict(case=tag, checks=len(rows), yardstick=ys, worst_ratio={k: v[0] for k, v in worst.items()},
                       worst_slice={k: v[1] for k, v in worst.items()}))
    print(f"\nLSTM-F64 {tag}: {len(rows)} checks; yardsticks " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(ys.items())))
    print(f"LSTM-F64 {tag}: worst err / yardstick " + ", ".join(f"{k} {v[0]:.2f} ({v[1]})" for k, v in sorted(worst.items())))
    assert not bad, f"{tag}: {len(bad)} of {len(rows)} over the gate: " + "; ".join(bad[:12])


def _refs(case, precision, grads):
    """(float64 reference, yardstick oracle).  The float64 and plain fp32 runs of a case are shared by all its tests (gradients included
    unless the case is forward-only); the bf16x3 yardstick computes gradients only where a bf16x3 backward is judged."""
    full = not CASES[case].get("forward_only", False)
    return _oracle(case, "f64", full), (_oracle(case, "x3", grads) if precision == "bf16x3" else _oracle(case, "fp32", full))


# ------------------------------------------------------------------------------------------------ the cases
TRAIN_RUNS = [(c, "fp32") for c in "abcdefghij"] + [("f", "bf16x3")]
INFER_RUNS = [("c", "bf16x6"), ("c", "bf16x3"), ("f", "bf16x6"), ("k", "fp32"), ("m", "fp32")]


@pytest.mark.parametrize("case,precision", TRAIN_RUNS, ids=[f"{c}-{p}" for c, p in TRAIN_RUNS])
def test_bilstm_forward_and_gradients_vs_float64(monkeypatch, case, precision):
    """Hidden states and scores (inference and training mode) and every gradient of the case, per video / per gate block."""
    ref, yard = _refs(case, precision, True)
    _judge(f"{case}/{precision}", case, _hip(case, precision, True, monkeypatch), ref, yard, True)


@pytest.mark.parametrize("case,precision", INFER_RUNS, ids=[f"{c}-{p}" for c, p in INFER_RUNS])
def test_bilstm_inference_vs_float64(monkeypatch, case, precision):
    """Inference only: the split-bf16 arithmetics of cases c (projection on operand planes) and f (the wide recurrence's bf16x6 recurrent
    product; bf16x6 training keeps the exact-fp32 recurrence, so there is nothing else to run in that mode), the 1000-frame chain, and
    the 3 969-video batch of case m on the launch chain."""
    if case == "c":
        assert sum(CASES[case]["lens"]) >= 1024                          # (below that the planes are not taken)
    ref, yard = _refs(case, precision, False)
    _judge(f"{case}/{precision}/inference", case, _hip(case, precision, False, monkeypatch), ref, yard, False)


def test_launch_chain_saves_feed_wide_bptt_case_m_vs_float64(monkeypatch):
    """Case m in training mode: lstm_step_kernel writes the saves (gates, cell states, h_{t-1}) that lstm_wide_bwd_kernel reads.  Training-mode
    scores of all 3 969 videos, and dx of the first 64 and the last 64 videos (first and last group of 64, the last one a single video), under
    the gates of the other cases.  The float64 / fp32 gradient oracles run on those 128 videos alone: dx of a video depends on that video and its
    rows of cw only (the full-batch gradient oracles take most of a minute on the CPU)."""
    from summarizer_amd.models.dsn import DSN
    c, inp = CASES["m"], _inputs("m")
    lens, off = c["lens"], inp["off"]
    dev = torch.device("cuda:0")
    m = DSN(c["D"], c["H"], c["L"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in inp["w"].items()})
    m = m.to(dev)
    with Poison(monkeypatch):
        xg = torch.from_numpy(np.concatenate(inp["xs"])).to(dev).requires_grad_(True)
        s = m.score_packed(xg, lens)
        (s * torch.from_numpy(inp["cw"]).to(dev)).sum().backward()
        dx = xg.grad.cpu().numpy().astype(np.float64)
        got = dict(train_scores=s.detach().cpu().numpy().astype(np.float64),
                   dx=np.concatenate([dx[off[v]:off[v + 1]] for v in M_DX_VIDEOS]))
    ref, yard = ({"scores": _oracle("m", mode, False)["scores"], "dx": _oracle("m", mode, True, M_DX_VIDEOS)["dx"]} for mode in ("f64", "fp32"))
    sub = np.concatenate([[0], np.cumsum([lens[v] for v in M_DX_VIDEOS])])
    sl = [("scores", f"train_scores[video {v}, T={lens[v]}]", "train_scores", "scores", (slice(off[v], off[v + 1]),), False) for v in range(len(lens))]
    sl += [("dx", f"dx[video {v}, T={lens[v]}]", "dx", "dx", (slice(sub[i], sub[i + 1]),), True) for i, v in enumerate(M_DX_VIDEOS)]
    _judge("m/fp32/training", "m", got, ref, yard, True, sl)


_CHILD = r'''
import sys
sys.path[:0] = [".", "tests", "tests/golden"]
import numpy as np, pytest
import test_gpu_lstm_f64 as T
from summarizer_amd import kernels
out = T._hip(sys.argv[2], "fp32", True, pytest.MonkeyPatch())
kernels.health_check()
np.savez(sys.argv[1], **out)
'''


def test_launch_per_step_kernels_case_d_vs_float64(tmp_path):
    """Case l: case d in a child process with SUMK_LSTM_PERSIST=0 -- lstm_step_kernel / lstm_bwd_step_kernel at H <= 256, which the
    library runs on a partitioned device and calls "same arithmetic": the same float64 gates."""
    f = tmp_path / "l.npz"
    r = subprocess.run([sys.executable, "-c", _CHILD, str(f), "d"], env=dict(os.environ, SUMK_LSTM_PERSIST="0"),
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref, yard = _refs("d", "fp32", True)
    _judge("l (d, SUMK_LSTM_PERSIST=0)", "d", dict(np.load(f)), ref, yard, True)
