"""CPU only: what the float64 gates of tests/test_gpu_sumgan_lstm_f64.py see.  A hand-written fp32 forward + BPTT in the kernels' own
structure (sumgan_lstm_f64_common.standin_layer / standin_decoder: torch.sigmoid / torch.tanh, plain products -- neither the yardstick
oracle nor autograd) stands in for the kernels.  It passes every gate of every case; each of seven planted errors, a few lines in the
stand-in, is rejected by the gate meant for it.  The gates of tests/test_gpu_sumgan_full.py (2e-5 absolute on the rows and final states
of a video, 3e-4 x max |ref| on dx per video, dh0 / dc0 per layer and video, and each WHOLE parameter tensor) are applied to the same
arrays and what they say is asserted too.

Measured here (worst error / yardstick of the kind the error is planted in; the gate is 4):
  planted error                                             case   kind         ratio    the old gates
  1 one gate block of dW_hh off by a relative 1e-4          Le     dweight_hh   2.5e2    pass   (1e-4 < 3e-4 of the whole tensor)
  2 a video's last step missing from dW_ih                  Le     dweight_ih   3.8e5    reject (dweight_ih_l0 2.3e-1; nothing else)
  3 dc0 without the final multiplication by the forget gate Ld     dc0          5.9e6    reject (dc0 of every video, 0.8 .. 1.3)
  4 h0 ignored for one video                                Ld     hidden_l0    1.2e6    reject (the video's rows 6.6e-2)
  5 dh_last added one step early for a shorter video        Le     dx           9.7e5    reject (the video's dx 5.0e-1)
  6 decoder layer 0 fed h_top[t] instead of h_top[t - 1]    Da     out          2.5e5    reject (every video's rows 4e-3 .. 9e-3)
  7 decoder top layer's backward without layer 0's W_ih     De2    dweight_ih   1.9e5    reject (dh0 / dc0 1.5e-2 .. 9e-2)
The smallest ratio is error 1's: 249 / 4 = 62 times its gate, which caps the multiplier at about 250 -- 4 leaves a factor 60.  The
stand-in itself lands at 0.3 .. 3.2 times the yardstick over all cases and kinds.  Of the seven, the old gates let error 1 through; what
else lies between the two sets of gates (old: pass, new: reject) is shown by test_errors_between_the_old_gates_and_the_new: one video's
h_n off by 1e-6, one video's dc0 off by a relative 1e-5, one gate block of a bias gradient off by a relative 1e-4."""
import functools

import numpy as np
import pytest
import torch

import sumgan_lstm_f64_common as S

STATE_GATE, GRAD_GATE = 2e-5, 3e-4                 # tests/test_gpu_sumgan_full.py
ALL = sorted(S.LAYER_CASES) + sorted(S.DECODER_CASES)


@pytest.mark.parametrize("case", ALL)
def test_every_case_reaches_its_path(case):
    S.check_regime(case)


def _old_gates(slices, got, ref):
    """What tests/test_gpu_sumgan_full.py would say: [(name, error, gate)] of what is over its gates.  Its slices are ours, except that a
    parameter gradient is judged as one tensor."""
    bad, seen = [], set()
    for kind, name, gk, rk, idx, rel in slices:
        if rk.split("_l")[0] in S.PARAMS:
            if gk in seen:
                continue
            seen.add(gk)
            name, idx = "d" + rk, (Ellipsis,)
        e = float(np.abs(got[gk][idx] - ref[rk][idx]).max()) / (float(np.abs(ref[rk][idx]).max()) if rel else 1.0)
        gate = GRAD_GATE if rel else STATE_GATE
        if not e <= gate:
            bad.append((name, e, gate))
    return bad


def _verdict(tag, slices, got, ref, yard):
    rec, bad = S.judge(f"host/{tag}", slices, got, ref, yard, quiet=True)
    old = _old_gates(slices, got, ref)
    print(f"\nSUMGAN-LSTM-F64-HOST {tag}: new gates {'reject' if bad else 'pass'} ({len(bad)} slices); worst ratio per kind "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(rec["worst_ratio"].items()))
          + f"; old gates {'reject' if old else 'pass'} " + ", ".join(f"{n} {e:.2e}" for n, e, g in old[:6]))
    return rec, bad, old


def _layer_verdict(case, tag, got):
    ref, yard = S.layer_refs(case, "fp32")
    return _verdict(f"{case}/{tag}", S.layer_slices(case), got, ref, yard)


def _decoder_verdict(case, state, tag, got):
    ref, yard = S.decoder_refs(case, state)
    return _verdict(f"{case}/{tag}", S.decoder_slices(case), got, ref, yard)


# ------------------------------------------------------------------------------------------------ the stand-in passes every case
@pytest.mark.parametrize("case", sorted(S.LAYER_CASES))
def test_layer_stand_in_passes_every_gate(case):
    slices = S.layer_slices(case)
    S.assert_reference_nowhere_zero(case, slices, S.layer_oracle(case, "f64"))
    rec, bad, old = _layer_verdict(case, "stand-in", S.standin_layer(case))
    assert not bad and not old, (bad[:5], old[:5])
    if case in ("Le", "Lg"):                       # the bf16x3 yardstick: the fp32 stand-in lies within it as well
        ref, yard = S.layer_refs(case, "bf16x3")
        rec3, bad3 = S.judge(f"host/{case}/stand-in vs x3", slices, S.standin_layer(case), ref, yard, quiet=True)
        assert not bad3 and all(rec3["yardstick"][k] > rec["yardstick"][k] for k in ("dx", "dweight_ih", "dweight_hh")), (bad3[:5], rec3, rec)


@pytest.mark.parametrize("state", [True, False], ids=["state", "zero-state"])
@pytest.mark.parametrize("case", sorted(S.DECODER_CASES))
def test_decoder_stand_in_passes_every_gate(case, state):
    S.assert_reference_nowhere_zero(case, S.decoder_slices(case), S.decoder_oracle(case, state, "f64"))
    rec, bad, old = _decoder_verdict(case, state, "stand-in" + ("" if state else " zero state"), S.standin_decoder(case, state))
    assert not bad and not old, (bad[:5], old[:5])


# ------------------------------------------------------------------------------------------------ planted errors
def _short_video(case):
    """A video of more than two and fewer than the most steps."""
    c = S.LAYER_CASES[case]
    return next(v for v, T in enumerate(c["lens"]) if 2 < T < c["tmax"])


@functools.lru_cache(maxsize=None)
def _mutant(n):
    """(kind the error is planted in, record, over the new gates, over the old gates) of planted error n."""
    if n == 1:
        return ("dweight_hh",) + _layer_verdict("Le", "1 dW_hh block f x (1 + 1e-4)", S.standin_layer("Le", "dwhh_block", block=1))
    if n == 2:
        v = _short_video("Le")
        return ("dweight_ih",) + _layer_verdict("Le", f"2 dW_ih without video {v}'s last step", S.standin_layer("Le", "dwih_last_step", video=v))
    if n == 3:
        return ("dc0",) + _layer_verdict("Ld", "3 dc0 before the forget gate", S.standin_layer("Ld", "dc0_no_forget"))
    if n == 4:
        return ("hidden_l0",) + _layer_verdict("Ld", "4 h0 of video 3 ignored", S.standin_layer("Ld", "h0_ignored", video=3))
    if n == 5:
        v = _short_video("Le")
        return ("dx",) + _layer_verdict("Le", f"5 dh_last of video {v} one step early", S.standin_layer("Le", "dh_last_early", video=v))
    if n == 6:
        feed = S.standin_decoder("Da", True)["out"]
        got = S.standin_decoder("Da", True, "feed_same_step", feed=torch.from_numpy(feed).float())
        return ("out",) + _decoder_verdict("Da", True, "6 layer 0 fed h_top[t]", got)
    if n == 7:
        return ("dweight_ih",) + _decoder_verdict("De2", True, "7 top layer's backward without W_ih of layer 0", S.standin_decoder("De2", True, "top_misses_wih0"))
    raise KeyError(n)


def test_planted_1_one_gate_block_of_dw_hh_off_by_1e_4():
    kind, rec, bad, old = _mutant(1)
    assert bad and all(b.startswith("dweight_hh_l0[f]") for b in bad), bad
    assert not old                                  # 1e-4 of one block: under 3e-4 of the whole tensor


def test_planted_2_a_videos_last_step_missing_from_dw_ih():
    kind, rec, bad, old = _mutant(2)
    assert bad and all(b.startswith("dweight_ih_l0[") for b in bad), bad
    assert [n for n, _, _ in old] == ["dweight_ih_l0"]   # one row's term in 300: the whole-tensor gate sees it too


def test_planted_3_dc0_without_the_forget_gate():
    kind, rec, bad, old = _mutant(3)
    assert bad and all(b.startswith("dc0[") for b in bad), bad
    assert old and all(n.startswith("dc0[") for n, _, _ in old)


def test_planted_4_h0_ignored_for_one_video():
    kind, rec, bad, old = _mutant(4)
    assert rec["worst_slice"]["hidden_l0"].startswith(("h0[video 3,", "train_h0[video 3,")) and rec["worst_ratio"]["hidden_l0"] > S.FACTOR
    assert rec["worst_ratio"]["dh0"] > S.FACTOR and old


def test_planted_5_dh_last_added_one_step_early():
    kind, rec, bad, old = _mutant(5)
    v = _short_video("Le")
    assert bad and rec["worst_slice"]["dx"].startswith(f"dx[video {v},") and rec["worst_ratio"]["dx"] > S.FACTOR
    assert not any(b.startswith(("h1[", "h0[", "h_n", "c_n", "train_")) for b in bad)      # a backward error: the forward is untouched
    assert old


def test_planted_6_decoder_layer_0_fed_the_same_steps_top_row():
    kind, rec, bad, old = _mutant(6)
    assert rec["worst_ratio"]["out"] > S.FACTOR and any(b.startswith("out[") for b in bad) and old


def test_planted_7_decoder_top_layer_backward_without_layer_0s_w_ih():
    kind, rec, bad, old = _mutant(7)
    assert bad and not any(b.startswith("out[") for b in bad) and rec["worst_ratio"]["dweight_ih"] > S.FACTOR
    assert old


def test_smallest_margin_of_the_planted_errors():
    """The smallest ratio by which a planted error exceeds its gate caps the multiplier; the docstring's table comes from this print."""
    margin = {}
    for n in range(1, 8):
        kind, rec, bad, old = _mutant(n)
        margin[n] = rec["worst_ratio"][kind] / S.FACTOR
        print(f"SUMGAN-LSTM-F64-HOST planted {n}: {kind} {rec['worst_ratio'][kind]:.3g} x yardstick = {margin[n]:.3g} x gate; "
              f"old gates {'reject' if old else 'pass'}")
        assert bad and margin[n] > 1.0, (n, kind, rec["worst_ratio"])
    low = min(margin, key=margin.get)
    print(f"SUMGAN-LSTM-F64-HOST smallest margin: planted {low}, {margin[low]:.3g} x its gate (multiplier cap {margin[low] * S.FACTOR:.3g})")
    assert margin[low] > 10.0, margin               # the multiplier could grow tenfold before a planted error passes
    assert [n for n in margin if not _mutant(n)[3]] == [1]         # the planted errors the old gates let through


def test_errors_between_the_old_gates_and_the_new():
    """Below the old gates, over the new: one video's h_n off by 1e-6 (old gate 2e-5), one video's dc0 off by 1e-5 of its largest entry
    (3e-4), one gate block of a bias gradient off by 1e-4 of the block's largest entry (3e-4 of the tensor's)."""
    case = "Ld"
    H = S.LAYER_CASES[case]["H"]
    ref, base = S.layer_oracle(case, "f64"), S.standin_layer(case)
    for name, keys, idx, kind, delta in (("h_n + 1e-6", ("hn", "train_hn"), (0, 4), "h_n", 1e-6),
                                         ("dc0 + 1e-5 rel", ("dc0",), (0, 4), "dc0", 1e-5 * np.abs(ref["dc0"][0, 4]).max()),
                                         ("dbias_hh[g] + 1e-4 rel", ("bias_hh_l0",), (slice(2 * H, 3 * H),), "dbias",
                                          1e-4 * np.abs(ref["bias_hh_l0"][2 * H:3 * H]).max())):
        got = {k: a.copy() for k, a in base.items()}
        for k in keys:
            got[k][idx] += delta
        rec, bad, old = _layer_verdict(case, name, got)
        assert bad and rec["worst_ratio"][kind] > S.FACTOR and not old, (name, bad[:3], old[:3])
        assert all(k == kind or r <= S.FACTOR for k, r in rec["worst_ratio"].items())
