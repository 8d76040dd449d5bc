"""CPU only: what the float64 gates of tests/test_gpu_lstm_f64.py see and the earlier gates (scores 1e-4, hidden states 2e-5, whole-tensor
relative L2 3e-4) do not.  The fp32 yardstick oracle of a case (default c) with a planted error stands in for the kernels: one video's rows
off by 1e-6, the last k chunk of the recurrent product dropped for one unit of one video, a video reading its neighbour's state in one step.
usage: python scripts/probes/lstm_f64_sensitivity.py [case]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np, torch
import test_gpu_lstm_f64 as T
from oracle import torch_port

CASE = sys.argv[1] if len(sys.argv) > 1 else "c"
c, inp = T.CASES[CASE], T._inputs(CASE)
H, lens, off = c["H"], c["lens"], inp["off"]
ref, yard = T._refs(CASE, "fp32", True)
order = sorted(range(len(lens)), key=lambda i: -lens[i])


def run(hook):
    p = {k: torch.from_numpy(v).requires_grad_(True) for k, v in inp["w"].items()}
    xs = [torch.from_numpy(x).requires_grad_(True) for x in inp["xs"]]
    layers = torch_port.bilstm_stack_ref(xs, {k[4:]: v for k, v in p.items() if k.startswith("rnn.")}, gate_math="rcp_form", matmul=hook)
    s = torch_port.GATE_MATH["rcp_form"][0](torch.cat(layers[-1]) @ p["out.0.weight"].t() + p["out.0.bias"])[:, 0]
    out = {f"h{l}": torch.cat(v) for l, v in enumerate(layers)}; out["scores"] = s
    names = list(p)
    g = torch.autograd.grad((s * torch.from_numpy(inp["cw"])).sum(), xs + [p[n] for n in names])
    out["dx"] = torch.cat(g[:len(xs)]); out.update(zip(names, g[len(xs):]))
    return {k: v.detach().double().numpy() for k, v in out.items()}


def report(name, got):
    got = dict(got); got.update({"train_" + k: v for k, v in got.items() if k[0] == "h" or k == "scores"})
    n0 = len(T.REPORT)
    try:
        T._judge(name, CASE, got, ref, yard, True); verdict = "PASSES the float64 gates (!)"
    except AssertionError as e:
        verdict = "fails the float64 gates: " + str(e).split(":", 1)[1][:160]
    r = T.REPORT[-1]
    l2 = {k: float(np.linalg.norm(got[k] - ref[k]) / np.linalg.norm(ref[k])) for k in ref}
    print(f"== {name}\n   {verdict}\n   worst slice ratio per kind: " + ", ".join(f"{k} {v:.1f}" for k, v in r["worst_ratio"].items()))
    print(f"   old gates: max |d scores| {np.abs(got['scores'] - ref['scores']).max():.2e} (gate 1e-4), max |d h| {np.abs(got['h0'] - ref['h0']).max():.2e} (2e-5), "
          f"whole-tensor rel L2: scores {l2['scores']:.2e}, h {l2['h0']:.2e}, dx {l2['dx']:.2e}, worst parameter gradient {max(v for k, v in l2.items() if '.' in k):.2e} (gate 3e-4)")


base = run(None)
report("unperturbed fp32 oracle", base)

# 1: one video's rows of the fp32 result off by 1e-6 absolute
v = 5
g = {k: a.copy() for k, a in base.items()}
g["h0"][off[v]:off[v + 1]] += 1e-6; g["scores"][off[v]:off[v + 1]] += 1e-6; g["dx"][off[v]:off[v + 1]] += 1e-6
report(f"1: video {v}'s rows of h and scores + 1e-6 and dx + 1e-6", g)

# 2: the last k chunk (8 of H) of the recurrent product dropped for ONE unit (gate i of unit 17, forward direction)
w_fwd = torch.from_numpy(inp["w"]["rnn.weight_hh_l0"])
def drop(a, w, site):
    y = a @ w.t()
    if site == "hh" and w.shape == w_fwd.shape and torch.equal(w.detach(), w_fwd):
        fix = torch.zeros_like(y); fix[10:11, 17] = a[10:11, H - 8:] @ w[17, H - 8:]
        y = y - fix
    return y
report("2: last k chunk (8 of H) of h . W_hh dropped for one unit's input gate, forward direction, sorted row 10 (one video), every step", run(drop))

# 3: video i + 1's state used for video i in ONE step (forward direction, sorted rows)
def swap(step, row):
    n = {"hh_fwd": 0}
    def hook(a, w, site):
        if site == "hh" and torch.equal(w.detach(), w_fwd):
            t = n["hh_fwd"]; n["hh_fwd"] += 1
            if t == step:
                a = torch.cat([a[:row], a[row + 1:row + 2], a[row + 1:]])
        return a @ w.t()
    return hook
sl = [lens[i] for i in order]
r2 = next(r for r in range(len(sl) - 1) if sl[r] == 2 and sl[r + 1] == 2)
r12 = next(r for r in range(len(sl) - 1) if sl[r] == 12 and sl[r + 1] == 12)
for step, row in ((1, r2),):
    vid = order[row]
    report(f"3: at step {step} of the forward direction sorted row {row} (video {vid}, T={lens[vid]}) reads row {row + 1}'s h (video {order[row + 1]})", run(swap(step, row)))
