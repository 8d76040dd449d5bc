"""GPU: SumGAN's one-direction LSTM layer (sumk_lstm_layer_forward / _backward behind eLSTM and cLSTM) and step-wise decoder
(sumk_lstm_decoder_forward / _backward behind dLSTM) of csrc/lstm.hip against float64, video by video, layer by layer and gate block by
gate block -- the family tests/test_gpu_sumgan_full.py holds at the reference's sizes to fixed gates (2e-5 / 1e-4 absolute, 3e-4 of a
whole tensor).  Only this family runs lstm_dec_step_kernel / lstm_dec_bwd_step_kernel, the a1 / w1 operand pair and the xin save of
lstm_gemv_step_kernel, the dGb / wb / b_shift coupling of lstm_tgemv_partial_kernel, h0 / c0, dh_last / dc_last, the step t = -1 (dh0 /
dc0), lstm_last_state_kernel, dir_grad_tail at a precision other than fp32, and the nd = 1 layouts of lstm_step_kernel /
lstm_bwd_step_kernel.

Reference: oracle/torch_port.lstm_stack_ref / dlstm_ref in float64 (pinned against nn.LSTM by tests/test_oracle.py).  Yardstick: the
SAME oracle in fp32 with the roundings of the kernels that run the case, read from csrc/lstm.hip:
  gate formulas  lstm_gemv_step_kernel, lstm_step_kernel, lstm_dec_step_kernel: sigmoidf_ (1 / (1 + expf(-v))) and the library's tanhf;
                 lstm_cellbwd_kernel, lstm_bwd_step_kernel, lstm_dec_bwd_step_kernel: the saved gates and tanhf(c) -- GATE_MATH["rcp_sigmoid"];
  dX GEMM        sumk_lstm_layer_backward sums K = 4H gate columns in one MFMA accumulator chain (torch_port.LinearChainDx);
  bf16x3         Linear3 on the input projection with its dx and dW_ih, LinearDw3 on dW_hh (dir_grad_tail passes the layer's precision
                 to both weight-gradient products); the recurrent products and the BPTT stay fp32;
  bf16x6         advertised as fp32-grade: the plain fp32 yardstick;
  decoder        fp32 throughout (dir_grad_tail at its default precision), no dX GEMM.
Slices, kinds and the gate (HIP error <= 4 x the kind's yardstick, floored at 2^-23 of the slice's largest reference magnitude; no slice
skipped) are tests/sumgan_lstm_f64_common.py's; tests/test_sumgan_lstm_f64_host.py runs the same gates on the CPU against planted errors
(the smallest exceeds its gate 62 times) and shows which of them the old gates let through.

The loss is a fixed random-weighted sum over the top layer's rows, h_n and c_n (dh_out, dh_last and dc_last all live); the decoder's
over its top-layer rows.  Every case restates the path it is named for (check_regime: few, m-tiles, unit blocks, strips, n_ksplit, tile
configuration, from lstm_carve / dec_carve / tgemv_geom) and asserts it; runs a second time with uninitialised device allocations
poisoned (bit-identical), and is followed by kernels.health_check().  Every training case also runs under torch.no_grad() (the running
cstate, lstm_last_state_kernel's other branch: hidden states of EVERY layer, h_n, c_n) through the same gates.

One-direction layer (H, In, videos; fp32 unless said):
  La   40, 24,  5 (<= 7 steps), h0 / c0, dh0 / dc0   mat-vec path, lanes past H / 4 idle, one partial strip, n_ksplit 5, the step t = -1
  Lb  104, 32,  8 (GV_MAXB), no initial state        nullptr branches; n_ksplit 13: the 16-stride loop of lstm_cellbwd_kernel runs once
  Lc 1060, 64,  3 (<= 12), h0 / c0                   second k chunk (lanes 0..8), 5 strips (last 36 wide), n_ksplit 118 (last 28 rows)
  Ld   40, 24,  9, h0 / c0                           lstm_step_kernel / lstm_bwd_step_kernel at nd = 1; 5 unit blocks, n_jblk 2 (last 8 wide)
  Le  100, 48, 33, L = 2 (models._bilstm.lstm_stack) second m-tile of one video, 13 unit blocks (last 4), n_jblk 4 (last 4); fp32, bf16x3, bf16x6
  Lf 1028, 64,  9 (<= 6), h0 / c0                    K split over four waves with a tail
  Lg  256, 64, 66 (8 353 rows)                       projection on 128x128 tiles, third m-tile of two videos; fp32, bf16x3, bf16x6
  La and Ld also with want_d0 = False: every other gradient bit-identical.
Decoder (H, L, videos), each with and without h0 / c0 and with dh0 / dc0 requested and not:
  Da   40, 2,  4 (T = 1 among them)  mat-vec path, both operand pairs, the xin save, b_shift 1 and 0
  Db  104, 1,  8                     L = 1: the top layer is layer 0 and feeds itself
  Dc 1060, 2,  2 (<= 10)             second k chunk, partial strip, partial last k split
  Dd   40, 3,  9                     lstm_dec_step_kernel / lstm_dec_bwd_step_kernel, a middle layer
  De  100, 1 and 2, 33               second m-tile, partial unit and column blocks
  Df 1028, 2,  9 (<= 6)              K split with a tail

Figures, measured on MI355X (worst HIP error / yardstick per kind, 4 is the limit; the poisoned re-runs are bit-identical, and so are the
want_d0 = False runs in everything but dh0 / dc0; the same numbers with slices and yardsticks in profiles/sumgan_lstm_f64_report.json):
  layer       hidden_l0 hidden_l1   h_n   c_n    dx   dh0   dc0  dweight_ih  dweight_hh  dbias
  La fp32          1.22            0.86  0.93  1.56  0.45  0.92        0.91        1.23   0.91
  Lb fp32          1.12            1.10  1.04  1.44                    1.64        1.22   0.83
  Lc fp32          0.82            0.91  0.81  3.07  0.09  0.48        0.82        0.99   0.79
  Ld fp32          0.89            1.16  0.93  1.30  0.45  0.69        0.95        1.26   1.06
  Le fp32          0.96      0.97  0.90  0.97  2.27  0.58  1.09        0.85        1.05   1.05
  Le bf16x3        1.00      1.00  0.99  0.99  0.99  1.01  1.09        0.98        1.03   1.02
  Le bf16x6        0.83      0.98  0.78  0.75  1.19  0.53  1.06        0.48        0.82   1.26
  Lf fp32          1.29            1.12  0.94  1.59  0.45  0.58        0.79        1.09   0.74
  Lg fp32          1.00            0.85  0.82  1.20                    0.92        1.79   1.13
  Lg bf16x3        1.00            1.00  1.00  1.01                    1.00        0.97   0.99
  Lg bf16x6        0.78            0.92  0.59  1.01                    0.92        1.53   1.01
  decoder (h0 / c0 | none)    out          dh0          dc0        dweight_ih   dweight_hh   dbias
  Da                      1.00 | 1.25  0.40 | 0.48  0.49 | 0.76  0.72 | 1.39  0.94 | 1.00  1.48 | 1.19
  Db                      0.94 | 0.86  0.34 | 0.32  0.69 | 0.78  1.27 | 1.10  0.93 | 1.10  1.33 | 0.55
  Dc                      1.11 | 1.00  0.11 | 0.07  0.15 | 0.09  0.24 | 0.28  0.23 | 0.32  0.28 | 0.29
  Dd                      1.00 | 1.12  0.51 | 0.60  0.87 | 0.67  1.11 | 0.81  1.05 | 0.78  0.83 | 0.77
  De (L = 1)              0.94 | 0.77  0.34 | 0.28  0.77 | 0.88  0.98 | 0.72  1.52 | 0.72  0.67 | 1.00
  De (L = 2)              0.82 | 1.00  0.43 | 0.37  0.47 | 0.33  1.06 | 1.03  0.77 | 0.89  0.77 | 1.12
  Df                      1.14 | 1.02  0.33 | 0.38  0.46 | 0.47  0.48 | 1.27  0.47 | 1.28  0.64 | 1.17
  Yardsticks, fp32: hidden states / h_n / c_n 3e-8 .. 1.2e-7, decoder rows 8e-9 .. 9e-8, gradients 1.6e-7 .. 2.3e-6 of a slice's largest
  entry; bf16x3: states 4e-7 .. 2.2e-6, gradients 3.8e-6 .. 9.2e-6.  5 494 slices in 41 judged runs; no kernel exceeded the gate (the
  largest ratio is dx of case Lc, 3.07: three videos, K = 4 240 in one accumulator chain).  The whole file, CPU references included,
  ran in 14.4 s.
"""
import json
import os

import numpy as np
import pytest
import torch

import sumgan_lstm_f64_common as S
from test_gpu_poison import Poison

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report():
    n0 = len(S.REPORT)
    yield
    rep = S.REPORT[n0:]
    for r in rep:
        print("SUMGAN-LSTM-F64-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "sumgan_lstm_f64.json"), "w") as f:
            json.dump(rep, f, indent=1)


@pytest.fixture(autouse=True)
def _health():
    yield
    from summarizer_amd import kernels
    kernels.health_check()


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _np(d):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in d.items() if v is not None}


def _same(a, b, what, but=()):
    assert sorted(k for k in a if k not in but) == sorted(k for k in b if k not in but), what
    for k in a:
        if k not in but:
            assert np.isfinite(b[k]).all() and np.array_equal(a[k], b[k]), f"{what}: {k} differs by {np.abs(a[k] - b[k]).max()}"


# ------------------------------------------------------------------------------------------------ the HIP side
def _hip_layer(case, precision, want_d0=True):
    """The case through kernels.lstm_layer_forward layer by layer under no_grad (h<l>, hn, cn), then in training mode with every gradient
    of the loss: L = 1 through kernels.lstm_layer_forward / lstm_layer_backward themselves, L = 2 through models._bilstm.lstm_stack and
    autograd (whose no_grad form must equal the layer-by-layer run bit for bit).  {name: float64 array}."""
    from summarizer_amd import kernels
    from summarizer_amd.models._bilstm import lstm_stack
    dev = _dev()
    c, inp = S.LAYER_CASES[case], S.layer_inputs(case)
    H, L, lens = c["H"], c["L"], c["lens"]
    sb = kernels.SeqBatch.get(lens, dev)
    w = {k: v.to(dev) for k, v in inp["w"].items()}
    weights = lambda l: tuple(w[f"{t}_l{l}"] for t in S.PARAMS)
    x = torch.cat(inp["xs"]).to(dev)
    h0, c0 = (inp["h0"].to(dev), inp["c0"].to(dev)) if c["state"] else (None, None)
    st = lambda s, l: None if s is None else s[l].contiguous()
    cw_out, cw_h, cw_c = inp["cw_out"].to(dev), inp["cw_h"].to(dev), inp["cw_c"].to(dev)
    out = {}
    with torch.no_grad():
        h, hn, cn = x, [], []
        for l in range(L):
            h, hl, cl, ws = kernels.lstm_layer_forward(h, sb, weights(l), H, st(h0, l), st(c0, l), training=False, precision=precision)
            assert ws is None
            out[f"h{l}"] = h
            hn.append(hl); cn.append(cl)
        out.update(hn=torch.stack(hn), cn=torch.stack(cn))
    if L == 1:
        h, hl, cl, ws = kernels.lstm_layer_forward(x, sb, weights(0), H, st(h0, 0), st(c0, 0), training=True, precision=precision)
        grads = [torch.zeros_like(t) for t in weights(0)]
        dx, dh0, dc0 = kernels.lstm_layer_backward(x, h, cw_out, cw_h[0], cw_c[0], sb, weights(0), st(c0, 0), grads, H, ws, True,
                                                   want_d0 and c["state"], precision=precision)
        out.update(train_h0=h, train_hn=hl[None], train_cn=cl[None], dx=dx)
        out.update({f"{t}_l0": g for t, g in zip(S.PARAMS, grads)})
        if want_d0 and c["state"]:
            out.update(dh0=dh0[None], dc0=dc0[None])
        else:
            assert dh0 is None and dc0 is None
    else:
        lstm = torch.nn.LSTM(c["In"], H, num_layers=L)
        lstm.load_state_dict(inp["w"])
        lstm = lstm.to(dev)
        with torch.no_grad():
            o, hn2, cn2 = lstm_stack(lstm, x, sb, h0, c0, precision=precision)
            assert torch.equal(o, out[f"h{L - 1}"]) and torch.equal(hn2, out["hn"]) and torch.equal(cn2, out["cn"])
        xg = x.clone().requires_grad_(True)
        h0g, c0g = (h0.clone().requires_grad_(want_d0), c0.clone().requires_grad_(want_d0)) if c["state"] else (None, None)
        o, hn2, cn2 = lstm_stack(lstm, xg, sb, h0g, c0g, precision=precision)
        ((o * cw_out).sum() + (hn2 * cw_h).sum() + (cn2 * cw_c).sum()).backward()
        out.update({f"train_h{L - 1}": o, "train_hn": hn2, "train_cn": cn2, "dx": xg.grad})
        out.update({k: prm.grad for k, prm in lstm.named_parameters()})
        if c["state"] and want_d0:
            out.update(dh0=h0g.grad, dc0=c0g.grad)
    return _np(out)


def _hip_decoder(case, state, want_d0):
    """kernels.lstm_decoder_forward / lstm_decoder_backward on the case; {name: float64 array}: out, dh0 / dc0 when requested, the
    state_dict names."""
    from summarizer_amd import kernels
    dev = _dev()
    c, inp = S.DECODER_CASES[case], S.decoder_inputs(case)
    H, L = c["H"], c["L"]
    sb = kernels.SeqBatch.get(c["lens"], dev)
    w = {k: v.to(dev) for k, v in inp["w"].items()}
    layers = [tuple(w[f"{t}_l{l}"] for t in S.PARAMS) for l in range(L)]
    grads = [tuple(torch.zeros_like(t) for t in ws) for ws in layers]
    h0, c0 = (inp["h0"].to(dev).contiguous(), inp["c0"].to(dev).contiguous()) if state else (None, None)
    out, ws = kernels.lstm_decoder_forward(sb, layers, H, h0, c0)
    dh0, dc0 = kernels.lstm_decoder_backward(sb, layers, H, c0, out, inp["cw"].to(dev), grads, ws, want_d0)
    assert (dh0 is None and dc0 is None) != want_d0
    got = dict(out=out, dh0=dh0, dc0=dc0)
    for l in range(L):
        got.update({f"{t}_l{l}": g for t, g in zip(S.PARAMS, grads[l])})
    return _np(got)


# ------------------------------------------------------------------------------------------------ the cases
LAYER_RUNS = [(c, "fp32") for c in sorted(S.LAYER_CASES)] + [("Le", "bf16x3"), ("Le", "bf16x6"), ("Lg", "bf16x3"), ("Lg", "bf16x6")]


@pytest.mark.parametrize("case,precision", LAYER_RUNS, ids=[f"{c}-{p}" for c, p in LAYER_RUNS])
def test_lstm_layer_forward_and_gradients_vs_float64(monkeypatch, case, precision):
    """Hidden states of every layer, h_n, c_n under no_grad; the top layer's rows, h_n, c_n and every gradient (dx per video, dh0 / dc0 per
    layer and video, every parameter per gate block) in training mode.  La, Ld: again with want_d0 = False."""
    S.check_regime(case)
    ref, yard = S.layer_refs(case, precision)
    slices = S.layer_slices(case)
    S.assert_reference_nowhere_zero(case, slices, ref)
    got = _hip_layer(case, precision)
    with Poison(monkeypatch):
        _same(got, _hip_layer(case, precision), f"{case}/{precision} under poisoned scratch")
    S.assert_judged(f"{case}/{precision}", slices, got, ref, yard)
    if case in ("La", "Ld"):
        assert S.LAYER_CASES[case]["state"]
        no_d0 = _hip_layer(case, precision, want_d0=False)
        assert "dh0" not in no_d0 and "dc0" not in no_d0
        _same(got, no_d0, f"{case} want_d0 = False", but=("dh0", "dc0"))
        with Poison(monkeypatch):
            _same(no_d0, _hip_layer(case, precision, want_d0=False), f"{case} want_d0 = False under poisoned scratch")
        S.assert_judged(f"{case}/{precision}/no d0", S.layer_slices(case, want_d0=False), no_d0, ref, yard)


DECODER_RUNS = [(c, s) for c in sorted(S.DECODER_CASES) for s in (True, False)]


@pytest.mark.parametrize("case,state", DECODER_RUNS, ids=[f"{c}-{'state' if s else 'zero-state'}" for c, s in DECODER_RUNS])
def test_lstm_decoder_forward_and_gradients_vs_float64(monkeypatch, case, state):
    """The decoder's top-layer rows per video, dh0 / dc0 per layer and video, every parameter gradient per layer and gate block; with
    h0 / c0 and without (nullptr: zeros), with dh0 / dc0 requested and not (every other gradient bit-identical)."""
    S.check_regime(case)
    ref, yard = S.decoder_refs(case, state)
    slices = S.decoder_slices(case)
    S.assert_reference_nowhere_zero(case, slices, ref)
    tag = f"{case}/{'state' if state else 'zero state'}"
    got = _hip_decoder(case, state, True)
    with Poison(monkeypatch):
        _same(got, _hip_decoder(case, state, True), f"{tag} under poisoned scratch")
    S.assert_judged(tag, slices, got, ref, yard)
    no_d0 = _hip_decoder(case, state, False)
    _same(got, no_d0, f"{tag} want_d0 = False", but=("dh0", "dc0"))
    with Poison(monkeypatch):
        _same(no_d0, _hip_decoder(case, state, False), f"{tag} want_d0 = False under poisoned scratch")
    S.assert_judged(f"{tag}/no d0", S.decoder_slices(case, want_d0=False), no_d0, ref, yard)
