"""CPU only: what the float64 gates of tests/test_gpu_gru_f64.py see.  An fp32 run of oracle/torch_port.bigru_stack_ref on case c (140
videos, H = 256, the kernels' gate formulas; its dX product a plain BLAS product, where the yardstick walks one accumulator chain, so it
is not the yardstick itself) stands in for the kernels.  It passes every gate; each of six planted errors is rejected by the gate meant
for it.  The earlier gates of tests/test_gpu_gru_persist.py (hidden states 2e-5, scores 1e-4, gradients 3e-4 x max |ref| per whole
parameter tensor and per video's dx) are applied to the same arrays, and what they say is asserted too: the figures stand in the
docstring of tests/test_gpu_gru_f64.py.  Every case's regime (group size, units per member, counter layout) is checked against the
plan restated in tests/gru_f64_common.py."""
import numpy as np
import pytest
import torch

import gru_f64_common as G
from oracle import torch_port

CASE = "c"
H_GATE, S_GATE, G_GATE = 2e-5, 1e-4, 3e-4          # tests/test_gpu_gru_persist.py


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_every_case_reaches_its_regime(case):
    G.check_regime(case)
    G.inputs(case)                                   # a one-frame video, a two-frame video and a tie in every batch of more than three


def _stand_in(hook=None):
    got = G.run_oracle(CASE, "fp32", True, hook)
    got.update({"train_" + k: v for k, v in got.items() if k[0] == "h" or k == "scores"})
    return got


def _old_gates(got, ref):
    """What tests/test_gpu_gru_persist.py would say: [(name, error, gate)] of what is over its gates."""
    c, off = G.CASES[CASE], G.inputs(CASE)["off"]
    bad = []
    for v in range(len(c["lens"])):
        rows = slice(off[v], off[v + 1])
        for name, key, gate, rel in ((f"h[video {v}]", "h0", H_GATE, False), (f"scores[video {v}]", "scores", S_GATE, False),
                                     (f"dx[video {v}]", "dx", G_GATE, True)):
            e = float(np.abs(got[key][rows] - ref[key][rows]).max()) / (float(np.abs(ref[key][rows]).max()) if rel else 1.0)
            if not e <= gate:
                bad.append((name, e, gate))
    for k in ref:
        if "." in k:
            e = float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max())
            if not e <= G_GATE:
                bad.append((k, e, G_GATE))
    return bad


@pytest.fixture(scope="module")
def world():
    c, inp = G.CASES[CASE], G.inputs(CASE)
    ref, yard = G.refs(CASE, "fp32", True)
    order = sorted(range(len(c["lens"])), key=lambda i: -c["lens"][i])
    return dict(c=c, inp=inp, ref=ref, yard=yard, order=order, base=_stand_in(), sorted_lens=[c["lens"][i] for i in order])


def _verdict(name, got, w):
    rec, bad = G.judge(f"host/{name}", CASE, got, w["ref"], w["yard"], True, quiet=True)
    old = _old_gates(got, w["ref"])
    print(f"\nGRU-F64-HOST {name}: new gates {'reject' if bad else 'pass'} ({len(bad)} slices); worst ratio per kind "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(rec["worst_ratio"].items()))
          + f"; old gates {'reject' if old else 'pass'} " + ", ".join(f"{n} {e:.2e} (gate {g:g})" for n, e, g in old))
    return rec, bad, old


def test_fp32_oracle_passes_every_gate(world):
    rec, bad, old = _verdict("unperturbed", world["base"], world)
    assert not bad and not old, (bad[:5], old[:5])
    assert max(rec["worst_ratio"].values()) < G.FACTOR


def _is(w, t):
    return w is t or (w.shape == t.shape and torch.equal(w.detach(), t.detach()))


def _weights():
    inp = G.inputs(CASE)
    return {k: torch.from_numpy(v) for k, v in inp["w"].items()}


def test_mutant_1_b_hn_outside_the_reset_gate_for_one_unit(world, monkeypatch):
    """n = tanh(Gx_n + r * (h W_hn) + b_hn) for unit 17 of both directions (the kernel adds b_hh before it multiplies by r)."""
    H, u = world["c"]["H"], 17

    def cell(gx, hw, b_hh, h, sig, tanh):
        xr, xz, xn = gx.chunk(3, dim=-1)
        hr, hz, hn = (hw + b_hh).chunk(3, dim=-1)
        r, z = sig(xr + hr), sig(xz + hz)
        pre = xn + r * hn
        wrong = xn + r * hw[:, 2 * H:] + b_hh[2 * H:]
        pick = torch.zeros(H, dtype=torch.bool); pick[u] = True
        return (1.0 - z) * tanh(torch.where(pick, wrong, pre)) + z * h
    monkeypatch.setattr(torch_port, "_gru_cell", cell)
    rec, bad, old = _verdict("1 b_hn outside r*(...)", _stand_in(), world)
    assert any(b.startswith(("h0[", "train_h0[")) for b in bad) and rec["worst_ratio"]["hidden_l0"] > G.FACTOR
    assert rec["worst_ratio"]["dbias_hh"] > G.FACTOR and "drnn.bias_hh_l0[n]" in " ".join(bad)
    assert old                                        # a whole bias term in every step: the old hidden-state gate sees it too


def test_mutant_2_last_k_chunk_of_the_recurrent_product_dropped(world):
    """The last 8 of the 256 k of h . W_hh missing for unit 17 (its three gate columns), forward direction, sorted row 10 (one video),
    every step."""
    H, u, row = world["c"]["H"], 17, 10
    w_fwd = _weights()["rnn.weight_hh_l0"]
    vid = world["order"][row]

    def drop(a, w, site):
        y = a @ w.t()
        if site == "hh" and _is(w, w_fwd) and a.shape[0] > row:
            fix = torch.zeros_like(y)
            for q in range(3):
                fix[row, q * H + u] = a[row, H - 8:] @ w[q * H + u, H - 8:]
            y = y - fix
        return y
    rec, bad, old = _verdict("2 last k chunk dropped", _stand_in(drop), world)
    assert rec["worst_slice"]["hidden_l0"].endswith(f"[video {vid}, T={world['c']['lens'][vid]}, fwd]") and rec["worst_ratio"]["hidden_l0"] > G.FACTOR
    assert rec["worst_ratio"]["dweight_hh"] > G.FACTOR and any(b.startswith("drnn.weight_hh_l0[") for b in bad)
    assert old and not any(n.startswith("scores") for n, _, _ in old)  # 6e-3 on one unit: the old hidden-state gate of that video sees it; no score gate does


def test_mutant_3_two_frame_video_reads_its_neighbours_state(world):
    """In its last step (step 1) a two-frame video's recurrent product takes the state of the next sorted row, another two-frame video,
    forward direction (the hand-off buffer is indexed by video; the carried z * h_prev is a register and stays right)."""
    sl, order = world["sorted_lens"], world["order"]
    row = next(r for r in range(len(sl) - 1) if sl[r] == 2 and sl[r + 1] == 2)
    vid = order[row]
    w_fwd = _weights()["rnn.weight_hh_l0"]
    n = {"calls": 0}

    def swap(a, w, site):
        if site == "hh" and _is(w, w_fwd):
            n["calls"] += 1
            if n["calls"] == 2:                      # step 1
                a = torch.cat([a[:row], a[row + 1:row + 2], a[row + 1:]])
        return a @ w.t()
    rec, bad, old = _verdict("3 neighbour's state in the last step", _stand_in(swap), world)
    assert n["calls"] == world["c"]["tmax"]
    assert rec["worst_slice"]["hidden_l0"].endswith(f"[video {vid}, T=2, fwd]") and rec["worst_ratio"]["hidden_l0"] > G.FACTOR
    assert rec["worst_slice"]["scores"].endswith(f"scores[video {vid}, T=2]") and rec["worst_ratio"]["scores"] > G.FACTOR
    assert old                                        # a whole wrong state: 5e-2 in the video's hidden states, the old gates see it too


def test_mutant_4_n_block_of_dw_hh_from_dn_instead_of_dn_r(world, monkeypatch):
    """dW_hh's n rows = dn^T h_prev instead of (dn r)^T h_prev, reverse direction: the weight-gradient GEMM reading the n block of dGx
    where it should read the stored dGh block.  Forward values, dx and every other gradient are untouched."""
    H = world["c"]["H"]
    w_rev = _weights()["rnn.weight_hh_l0_reverse"]
    carry = {}

    def hook(a, w, site):
        if site == "hh" and _is(w, w_rev):
            # value a @ w.T; the state's gradient through the first term, the weight's through `extra` (worth exactly zero), which the
            # cell adds OUTSIDE r * (...) in the n block
            carry["extra"] = a.detach() @ w.t() - (a @ w.t()).detach()
            return a @ w.detach().t()
        return a @ w.t()

    def cell(gx, hw, b_hh, h, sig, tanh):
        extra = carry.pop("extra", None)
        xr, xz, xn = gx.chunk(3, dim=-1)
        hr, hz, hn = (hw + b_hh).chunk(3, dim=-1)
        if extra is not None:
            er, ez, en = extra.chunk(3, dim=-1)
            hr, hz, xn = hr + er, hz + ez, xn + en
        r, z = sig(xr + hr), sig(xz + hz)
        return (1.0 - z) * tanh(xn + r * hn) + z * h
    monkeypatch.setattr(torch_port, "_gru_cell", cell)
    got = _stand_in(hook)
    base = world["base"]
    k = "rnn.weight_hh_l0_reverse"
    assert all(np.array_equal(got[n], base[n]) for n in got if n != k) and np.array_equal(got[k][:2 * H], base[k][:2 * H])
    rec, bad, old = _verdict("4 dW_hh n block from dn", got, world)
    assert bad and all(b.startswith(f"d{k}[n]") for b in bad), bad
    assert any(n == k for n, _, _ in old)             # a whole block wrong by a factor 1 / r: the old whole-tensor gate sees it too


def test_mutant_5_one_videos_dx_rows_off_by_1e_6(world):
    v, off = 5, world["inp"]["off"]
    got = {k: a.copy() for k, a in world["base"].items()}
    got["dx"][off[v]:off[v + 1]] += 1e-6
    rec, bad, old = _verdict("5 dx rows + 1e-6", got, world)
    assert bad and all(b.startswith(f"dx[video {v},") for b in bad), bad
    assert not old


def test_mutant_6_reverse_direction_of_a_one_frame_video_starts_from_the_forward_state(world, monkeypatch):
    """The reverse direction of a one-frame video starts from that video's forward state instead of zero (state left over from the
    team's previous item: `hlast` / the hand-off tags not reset): both the recurrent product and the carried z * h_prev take it."""
    H, order, off = world["c"]["H"], world["order"], world["inp"]["off"]
    row = len(order) - 1
    vid = order[row]
    assert world["c"]["lens"][vid] == 1
    h_fwd = torch.from_numpy(world["base"]["h0"][off[vid], :H]).float()
    w_rev = _weights()["rnn.weight_hh_l0_reverse"]
    st = {"calls": 0}
    real = torch_port._gru_cell

    def hook(a, w, site):
        if site == "hh" and _is(w, w_rev):
            st["calls"] += 1
            if st["calls"] == 1:
                a = torch.cat([a[:row], h_fwd[None].to(a.dtype), a[row + 1:]])
                st["h"] = a
        return a @ w.t()

    def cell(gx, hw, b_hh, h, sig, tanh):
        return real(gx, hw, b_hh, st.pop("h", h), sig, tanh)
    monkeypatch.setattr(torch_port, "_gru_cell", cell)
    rec, bad, old = _verdict("6 one-frame video, reverse from the forward state", _stand_in(hook), world)
    assert st["calls"] == world["c"]["tmax"]
    assert rec["worst_slice"]["hidden_l0"].endswith(f"[video {vid}, T=1, rev]") and rec["worst_ratio"]["hidden_l0"] > G.FACTOR
    assert rec["worst_ratio"]["scores"] > G.FACTOR
    assert [n for n, _, _ in old if "." in n] == []   # one row in 1 720: every whole-tensor gradient passes the old gates


def test_errors_between_the_old_gates_and_the_new(world):
    """Mutants 1-4 and 6 move a hidden state by 6e-3 or more, which the old per-video hidden-state gate (2e-5) sees as well.  What only
    the new gates see lies below the old ones: one video's hidden states of one direction off by 1e-6 (old gate 2e-5), one video's
    scores off by 1e-6 (1e-4), one gate block of one bias gradient off by 1e-4 of the block's largest entry (3e-4 of the tensor's)."""
    off, H = world["inp"]["off"], world["c"]["H"]
    v = 7
    for name, key, idx, kind, delta in (("h rev + 1e-6", "h0", (slice(off[v], off[v + 1]), slice(H, 2 * H)), "hidden_l0", 1e-6),
                                        ("scores + 1e-6", "scores", (slice(off[v], off[v + 1]),), "scores", 1e-6),
                                        ("dbias_hh[n] rev + 1e-4 rel", "rnn.bias_hh_l0_reverse", (slice(2 * H, 3 * H),), "dbias_hh", None)):
        got = {k: a.copy() for k, a in world["base"].items()}
        got[key][idx] += delta if delta is not None else 1e-4 * np.abs(world["ref"][key][idx]).max()
        rec, bad, old = _verdict(name, got, world)
        assert bad and rec["worst_ratio"][kind] > G.FACTOR and not old, (name, bad[:3], old[:3])
        assert all(k == kind or r <= G.FACTOR for k, r in rec["worst_ratio"].items())
