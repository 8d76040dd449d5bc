"""GPU: the bidirectional GRU recurrences of DSN(cell="gru") -- the persistent forward and BPTT of csrc/gru_persist.hip in every regime
their plan can give a batch, the step path of csrc/gru.hip under models/_bilstm.GruLayerFunction, and the GEMMs around both in fp32,
bf16x6 and bf16x3 -- against float64, video by video and gate block by gate block.  The GRU twin of tests/test_gpu_lstm_f64.py.

tests/test_gpu_gru_persist.py and tests/test_gpu_gru.py hold hidden states to 2e-5, scores to 1e-4 and gradients to 3e-4 x max |ref|
per whole parameter tensor (stock fp32 sits about 30 x inside), launch one work item per team at the most, and never set `precision`.
Here the reference is oracle/torch_port.bigru_stack_ref in float64 (pinned against nn.GRU by tests/test_oracle.py) and the yardstick
is the SAME oracle in fp32 on the same inputs:

  quantity   hidden states of every layer (kernels.bigru_layer_forward, inference and training mode; the step path has one mode:
             GruLayerFunction without and with grad) per video and direction, scores (score_packed, both modes) per video: largest
             absolute error of the slice;
             gradients of sum(scores * cw), cw fixed random: dx per video, weight_ih / weight_hh / bias_ih / bias_hh per direction and
             per gate block (r, z, n: the three row thirds), the head's weight and bias: largest absolute error of the slice / largest
             reference magnitude of the slice.
  gate       HIP error <= 4 x yardstick.  Yardstick of a KIND (hidden states of a layer, scores, dx, weight_ih blocks, weight_hh blocks,
             bias_ih blocks, bias_hh blocks, head) = the largest |fp32 oracle - float64| over the case's slices of that kind, with a
             floor of 2 fp32 ulps (2^-23) of the slice's largest reference magnitude.  The factor 4 is the project's.
  fp32       persistent path: gate_math="rcp_form" (1 / (1 + exp(-v)), 1 - 2 / (1 + exp(2 v)): fast_sigmoid / fast_tanh of
             csrc/persist_common.h:20-21, called at gru_persist.hip:255-257).  Step path (case i): gate_math="exact" (gru.hip:14,25-27
             calls expf / tanhf).  The dX GEMM (gru_persist.hip:608-616, lstm.hip sumk_linear_backward) sums its K = 3H gate columns per
             direction in ONE fp32 MFMA accumulator (csrc/gemm_regstage.h); the yardstick takes that product as the kernel does
             (torch_port.LinearChainDx / mm_chain, shown on the CPU for the LSTM file: a BLAS product's error grows far slower with K).
  bf16x6     advertised as fp32-grade: the plain fp32 yardstick.
  bf16x3     a documented difference in arithmetic: the yardstick makes the hi.hi + hi.lo + lo.hi roundings (torch_port.mm3) in exactly
             the products the library runs in that mode.
             Persistent path: the input projection (gru_persist.hip:528 g.precision), dW_ih (:592), dW_hh's r, z rows (:596-597) and
             n rows (:599-600) -- gemm_tn_splitk_accum gets `precision` in all three launches -- and dX (:614): torch_port.Linear3 on
             site "ih", torch_port.LinearDw3 on site "hh".  The recurrent product (:189-196, :234-237) and the BPTT's dGh . W_hh
             (:441, :464-467) are fp32 MFMAs inside the kernels whatever the precision: LinearDw3 keeps both exact.
             Step path: kernels.linear_forward / linear_backward carry `precision` into every product (models/_bilstm.py:101 projection,
             :108 recurrent product, :141 dh = dGh . W_hh and dW_hh, :143 dX and dW_ih): Linear3 on both sites with its dx in bf16x3.
Every case asserts that training-mode and inference-mode hidden states are BIT-equal (the forward differs only in its saves:
gru_persist.hip:262-266), runs twice with bit-identical results, runs with uninitialised device allocations poisoned (Poison of
tests/test_gpu_sumgan_full.py) and is followed by kernels.health_check().  Each video has its own feature seed; every batch of more than
three videos holds a one-frame video, a two-frame video and a tie in length.  References are cached per (case, arithmetic).

Cases (H, In, L; videos; what the plan gives them -- asserted from pk_group_size / upm / pk_items_shard restated in
tests/gru_f64_common.py, so that a change of the plan cannot silently move a case off its path):
  a  256, 128, 1    9 (<= 64 frames)   groups of 3: M16 forms (16-row MFMAs), 6 items; fp32, bf16x6, bf16x3, forward and backward
  b  256, 128, 1   70 (<= 40)          groups of 18: 32-row forms, the last group partial (16), 8 items
  c  256, 128, 1  140 (<= 24)          groups of 32, 10 items on 8 teams: two teams run a second item (loaded_dir reuse, LDS
                                       re-initialisation, a second item's exchange buffer and step counter); fp32, bf16x3
  d  96 / 128 / 132 / 192, 64, 1   20 (<= 30)   3 / 4 / 5 / 6 units per member; H = 132: 27 members, the last with 2 units, H % 8 != 0
  e  100,  64, 2   20 (<= 30)          layer 1 has In = 2H = 200; 4 units per member, 25 members; fp32, bf16x3
  f   64,  64, 1   64 (<= 12)          four full 16-row groups: the last batch size of the M16 forms
  g  256,  64, 1    1 of 1000 frames   forward only: error growth over 1000 hand-offs
  h   64,  64, 1 2017 (1-3)            64 groups, 128 items: the unsharded BPTT step counter (item_words = 1, n_shards = 1), 16 items per
                                       team, the last group one video.  Scores of every video in both modes, dx of the first and the
                                       last 64 videos, every parameter gradient
  i  260,  64, 1   10 (<= 12)          step path (bigru_eligible false): gru_cell_fwd / bwd kernels + GEMMs with a k tail; fp32, bf16x3

Figures, measured on MI355X (worst HIP error / yardstick per kind, 4 is the limit):
  case          hidden  scores    dx  weight_ih  weight_hh  bias_ih  bias_hh  head     yardsticks: hidden / scores / dx
  a fp32          1.02    0.69  1.80       0.82       1.29     1.79     1.19  0.89     1.7e-7 / 8.7e-8 / 3.2e-7
  a bf16x6        0.97    0.80  1.38       0.69       0.85     1.96     0.99  0.64     (the fp32 yardsticks)
  a bf16x3        1.01    1.00  1.02       1.04       1.17     1.00     0.99  1.04     1.9e-6 / 4.3e-7 / 4.0e-6
  b fp32          1.00    0.96  1.13       0.95       1.28     1.53     1.46  0.31     1.9e-7 / 8.4e-8 / 5.9e-7
  c fp32          1.15    0.84  1.03       0.86       0.92     1.27     1.48  0.46     1.8e-7 / 9.2e-8 / 6.4e-7
  c bf16x3        0.96    1.00  1.00       0.98       0.93     1.02     1.03  1.03     2.1e-6 / 7.4e-7 / 6.3e-6
  d H 96          1.00    0.87  0.93       0.93       1.06     1.06     1.00  0.06     1.6e-7 / 7.7e-8 / 3.5e-7
  d H 128         0.96    0.81  1.12       0.94       0.78     0.90     0.88  0.45     1.6e-7 / 8.4e-8 / 3.6e-7
  d H 132         1.05    0.95  0.97       1.02       1.00     1.53     1.36  0.38     1.4e-7 / 7.4e-8 / 3.9e-7
  d H 192         1.03    0.92  1.39       1.15       0.88     0.80     1.11  0.59     1.3e-7 / 7.3e-8 / 3.8e-7
  e fp32 (L 2)    1.15    1.15  1.08       0.59       1.08     1.18     0.88  1.09     1.7e-7 / 7.1e-8 / 5.1e-7
  e bf16x3        1.00    1.00  1.12       0.98       1.20     1.03     0.96  1.08     2.2e-6 / 5.0e-7 / 9.2e-6
  f fp32          1.05    0.92  0.73       0.87       0.87     0.79     0.85  0.63     1.7e-7 / 7.6e-8 / 4.1e-7
  g fp32          1.12    0.81                                                         1.3e-7 / 8.7e-8 (forward only)
  h fp32                  0.95  0.98       1.56       0.94     1.54     1.03  0.25     9.0e-8 / 4.3e-7 (scores / dx; dx of 128 videos)
  i fp32          1.00    0.81  2.12       0.95       1.09     2.01     1.73  0.52     7.1e-8 / 6.2e-8 / 4.7e-7
  i bf16x3        1.01    0.84  0.95       1.00       1.00     1.01     1.04  1.01     1.3e-6 / 2.8e-7 / 7.1e-6
  Parameter-gradient yardsticks lie between 2.3e-7 and 6.4e-6 (fp32) and 2.5e-6 and 1.3e-5 (bf16x3).  No kernel exceeded the gate.  The
  bf16x3 ratios of 1.0 say that the yardstick multiplies where the library does (an fp32 result would sit at a tenth of it); each run in
  bf16x6 / bf16x3 also asserts that its bits differ from the fp32 run's, so that `precision` cannot be dropped on the way unnoticed.

What these gates see, shown on the CPU with an fp32 oracle run of case c standing in for the kernels (tests/test_gru_f64_host.py; worst
slice error / yardstick of the kind it was planted for):
  1  b_hn added outside r * (...) for one unit: hidden 2.8e4 x, bias_hh 1.8e5 x -- the old gates see it too (bias_hh gradient 0.15);
  2  the last 8-wide k chunk of h . W_hh dropped for one unit of one video: hidden 3.4e4 x, weight_hh 3.3e4 x -- hidden states of that
     video move by 6.2e-3, over the old 2e-5; its scores stay inside the old 1e-4;
  3  a two-frame video reading its neighbour's state in its last step: hidden 2.7e5 x, scores 1.3e4 x -- old gates see it (hidden 5e-2);
  4  the n block of dW_hh from dn instead of dn . r, one direction: weight_hh[n] of that direction 1.5e6 x and NO other slice moves
     -- the old whole-tensor gate sees it too (1.09 relative);
  5  one video's dx rows off by 1e-6: dx 65 x -- passes every old gate;
  6  the reverse direction of a one-frame video started from the forward state: hidden 7.9e5 x, scores 1.2e5 x -- old gates see the
     video's hidden states (0.15) and scores; every whole-tensor gradient gate passes (one row in 1 720);
  below the old gates and over the new: one video's hidden states of one direction + 1e-6 (6 x), one video's scores + 1e-6 (12 x), one
  gate block of one bias gradient off by 1e-4 of its largest entry (120 x).
The GRU's old gates are per video already, so what they miss is what is small: the new gates are 30 x tighter, per gate block, and hold
bf16x6 / bf16x3, the second work item, the unsharded counter and the units-per-member walk, which nothing ran before.
"""
import json
import os

import numpy as np
import pytest
import torch

import gru_f64_common as G
from test_gpu_sumgan_full import Poison

pytestmark = pytest.mark.gpu
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


@pytest.fixture(scope="module", autouse=True)
def _report():
    n0 = len(G.REPORT)
    yield
    mine = G.REPORT[n0:]
    for r in mine:
        print("GRU-F64-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "gru_f64.json"), "w") as f:
            json.dump(mine, f, indent=1)


@pytest.fixture(autouse=True)
def _health():
    yield
    from summarizer_amd import kernels
    kernels.health_check()


def _hip(case, precision, grads, monkeypatch):
    """Hidden states of every layer through kernels.bigru_layer_forward (the step path: models._bilstm.GruLayerFunction), as
    models._bilstm.bigru_scores runs the layers; scores through DSN.score_packed; with grads also both in training mode and every
    gradient.  {name: float64 array}."""
    from summarizer_amd import kernels
    from summarizer_amd.models import _bilstm
    from summarizer_amd.models.dsn import DSN
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    c, inp = G.CASES[case], G.inputs(case)
    H, D, L, lens = c["H"], c["D"], c["L"], c["lens"]
    step = c.get("step_path", False)
    G.check_regime(case)
    for l in range(L):                                                   # the path the model will take for every layer
        assert kernels.bigru_eligible(D if l == 0 else 2 * H, H) == (not step), (case, l)
    m = DSN(D, H, L, cell="gru")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in inp["w"].items()})
    m.precision = precision
    m = m.to(dev)
    x = torch.from_numpy(np.concatenate(inp["xs"])).to(dev)
    out = {}

    def layer(h, l, training):
        w = [p[f"rnn.{n}_l{l}{suf}"] for suf in ("", "_reverse") for n in NAMES]
        if step:
            return _bilstm.GruLayerFunction.apply(h, sb, H, precision, *w)
        return kernels.bigru_layer_forward(h, sb, [t.detach() for t in w], H, training=training, precision=precision)[0]

    with Poison(monkeypatch):
        sb = kernels.SeqBatch.get(lens, dev)
        p = dict(m.named_parameters())
        with torch.no_grad():
            h = x
            for l in range(L):
                h = out[f"h{l}"] = layer(h, l, False)
            out["scores"] = m.score_packed(x, lens)
        if grads:
            h = x
            for l in range(L):
                h = layer(h, l, True)                                    # (the step path: with grad, its saves kept)
                out[f"train_h{l}"] = h.detach()
            del h
            xg = x.clone().requires_grad_(True)
            s = m.score_packed(xg, lens)
            (s * torch.from_numpy(inp["cw"]).to(dev)).sum().backward()
            out["train_scores"], out["dx"] = s.detach(), xg.grad
            out.update({k: prm.grad for k, prm in m.named_parameters()})
        out = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in out.items()}
    return out


def _run(tag, case, precision, grads, monkeypatch):
    got = _hip(case, precision, grads, monkeypatch)
    again = _hip(case, precision, grads, monkeypatch)
    assert sorted(got) == sorted(again)
    for k in got:                                                        # a second run is bit-identical (NaN would fail here as well)
        assert np.array_equal(got[k], again[k]), (tag, k)
    if grads:
        for l in range(G.CASES[case]["L"]):                              # the training-mode forward differs only in its saves
            assert np.array_equal(got[f"h{l}"], got[f"train_h{l}"]), (tag, l)
    if precision != "fp32":                                              # `precision` reaches the GEMMs: other bits than fp32
        plain = _hip(case, "fp32", grads, monkeypatch)
        for k in ("h0", "dx", "rnn.weight_ih_l0", "rnn.weight_hh_l0"):
            assert not np.array_equal(got[k], plain[k]), (tag, k)
    ref, yard = G.refs(case, precision, grads)
    G.assert_judged(tag, case, got, ref, yard, grads)


TRAIN_RUNS = ([(c, "fp32") for c in ("a", "b", "c", "d96", "d128", "d132", "d192", "e", "f", "h", "i")]
              + [("a", "bf16x6"), ("a", "bf16x3"), ("c", "bf16x3"), ("e", "bf16x3"), ("i", "bf16x3")])


@pytest.mark.parametrize("case,precision", TRAIN_RUNS, ids=[f"{c}-{p}" for c, p in TRAIN_RUNS])
def test_bigru_forward_and_gradients_vs_float64(monkeypatch, case, precision):
    """Hidden states and scores (inference and training mode) and every gradient of the case, per video / per gate block."""
    _run(f"{case}/{precision}", case, precision, True, monkeypatch)


def test_bigru_1000_hand_offs_vs_float64(monkeypatch):
    """Case g, inference only: one video of 1000 frames."""
    _run("g/fp32/inference", "g", "fp32", False, monkeypatch)
