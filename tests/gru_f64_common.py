"""Shared by tests/test_gpu_gru_f64.py (the GRU kernels against float64) and tests/test_gru_f64_host.py (the same gates on the CPU, the
fp32 oracle and planted errors standing in for the kernels): the cases with the regime each must reach, their inputs, the float64
reference and the fp32 / bf16x3 yardstick oracles (oracle/torch_port.bigru_stack_ref), the slices and the gate.  Nothing here needs a
GPU or the library."""
import functools

import numpy as np
import torch

import recipes as R
from oracle import torch_port

ULP = 2.0 ** -24
FACTOR = 4.0
F64 = torch.float64
REPORT = []

_LENS_20 = [30, 1, 2, 17, 30, 9, 25, 4, 12, 17, 3, 28, 7, 21, 5, 14, 1, 19, 8, 26]
CASES = {
    "a": dict(H=256, D=128, L=1, lens=[64, 1, 2, 33, 64, 17, 33, 40, 5], tmax=64),
    "b": dict(H=256, D=128, L=1, lens=[40, 1, 2] + [(7 * i) % 40 + 1 for i in range(67)], tmax=40),
    "c": dict(H=256, D=128, L=1, lens=[24, 1, 2] + [(5 * i) % 24 + 1 for i in range(137)], tmax=24),
    "d96": dict(H=96, D=64, L=1, lens=_LENS_20, tmax=30),
    "d128": dict(H=128, D=64, L=1, lens=_LENS_20, tmax=30),
    "d132": dict(H=132, D=64, L=1, lens=_LENS_20, tmax=30),
    "d192": dict(H=192, D=64, L=1, lens=_LENS_20, tmax=30),
    "e": dict(H=100, D=64, L=2, lens=_LENS_20, tmax=30),
    "f": dict(H=64, D=64, L=1, lens=[12, 1, 2] + [(5 * i) % 12 + 1 for i in range(61)], tmax=12),
    "g": dict(H=256, D=64, L=1, lens=[1000], tmax=1000, forward_only=True),
    "h": dict(H=64, D=64, L=1, lens=[3, 1, 2] + [(i % 3) + 1 for i in range(2014)], tmax=3),
    "i": dict(H=260, D=64, L=1, lens=[12, 1, 2, 7, 12, 5, 9, 3, 7, 11], tmax=12, step_path=True),
}
H_DX_VIDEOS = tuple(range(64)) + tuple(range(2017 - 64, 2017))     # case h: the videos whose dx is judged
SEED = {c: 7300 + 100 * i for i, c in enumerate(sorted(CASES))}
GRU_TENSORS = (("weight_ih", "dweight_ih"), ("weight_hh", "dweight_hh"), ("bias_ih", "dbias_ih"), ("bias_hh", "dbias_hh"))


# ------------------------------------------------------------------------------------------------ the plan, restated
# csrc/persist_common.h: pk_group_size, pk_items_shard (PSTATE_WORDS = 16 + 16384, PSTATE_SPARE_WORDS = 512, PSTATE_ITEM_WORDS = 128),
# PK_TEAMS = 8; csrc/gru_persist.hip: upm / n_active (sumk_bigru_layer_forward), m16 = gsize <= 16; kernels.bigru_eligible.
def plan(H, In, n_seq):
    if not (0 < H <= 256 and H % 4 == 0 and In % 4 == 0):
        return dict(persistent=False)
    gsize = min(32, max(1, (2 * n_seq + 7) // 8))
    n_groups = (n_seq + gsize - 1) // gsize
    items = 2 * n_groups
    upm = min(8, (H + 31) // 32)
    n_active = (H + upm - 1) // upm
    return dict(persistent=True, gsize=gsize, n_groups=n_groups, items=items, m16=gsize <= 16, last_group=n_seq - (n_groups - 1) * gsize,
                sharded=items * 128 <= 16384 - 512, upm=upm, n_active=n_active, last_units=H - (n_active - 1) * upm,
                max_items_per_team=(items + 7) // 8)


# what each case must reach (the table of the test's docstring): a change of the plan that moves a case off its path fails here
REGIME = {
    "a": dict(gsize=3, m16=True, items=6, upm=8, n_active=32, sharded=True),
    "b": dict(gsize=18, m16=False, items=8, last_group=16, max_items_per_team=1, sharded=True),
    "c": dict(gsize=32, m16=False, items=10, last_group=12, max_items_per_team=2, sharded=True),
    "d96": dict(upm=3, n_active=32, last_units=3, m16=True),
    "d128": dict(upm=4, n_active=32, last_units=4, m16=True),
    "d132": dict(upm=5, n_active=27, last_units=2, m16=True),
    "d192": dict(upm=6, n_active=32, last_units=6, m16=True),
    "e": dict(upm=4, n_active=25, m16=True, items=8),
    "f": dict(gsize=16, m16=True, n_groups=4, last_group=16, items=8),
    "g": dict(gsize=1, m16=True, items=2, upm=8),
    "h": dict(gsize=32, n_groups=64, items=128, sharded=False, max_items_per_team=16, last_group=1),
    "i": dict(persistent=False),
}


def check_regime(case):
    c = CASES[case]
    got = plan(c["H"], c["D"], len(c["lens"]))
    want = REGIME[case]
    assert got["persistent"] == (not c.get("step_path", False)), (case, got)
    assert {k: got[k] for k in want} == want, (case, got, want)
    if case == "d132":
        assert c["H"] % 8 != 0
    if case == "i":
        assert c["H"] % 32 != 0 and c["H"] % 8 != 0              # a k tail in every GEMM over H
    if c["L"] > 1:                                                # layer 1 (In = 2H) runs the same plan
        assert plan(c["H"], 2 * c["H"], len(c["lens"])) == got
    return got


def gru_weights(D, H, L, seed):
    """nn.GRU(bidirectional=True) + Linear(2H, 1) state_dict names of DSN(cell="gru"), seeded (recipes.lstm_weights' ranges)."""
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    p = {}
    for l in range(L):
        In = D if l == 0 else 2 * H
        for suf in ("", "_reverse"):
            p[f"rnn.weight_ih_l{l}{suf}"] = rng.uniform(-k, k, (3 * H, In)).astype(np.float32)
            p[f"rnn.weight_hh_l{l}{suf}"] = rng.uniform(-k, k, (3 * H, H)).astype(np.float32)
            p[f"rnn.bias_ih_l{l}{suf}"] = rng.uniform(-k, k, (3 * H,)).astype(np.float32)
            p[f"rnn.bias_hh_l{l}{suf}"] = rng.uniform(-k, k, (3 * H,)).astype(np.float32)
    kh = 1.0 / np.sqrt(2 * H)
    p["out.0.weight"] = rng.uniform(-kh * 3, kh * 3, (1, 2 * H)).astype(np.float32)
    p["out.0.bias"] = rng.uniform(-kh, kh, (1,)).astype(np.float32)
    return p


# ------------------------------------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def inputs(case):
    """Weights, one feature block per video (its own seed) and the fixed loss weights of a case."""
    c = CASES[case]
    lens, seed = c["lens"], SEED[case]
    if len(lens) > 3:
        assert 1 in lens and 2 in lens and len(set(lens)) < len(lens), case
    assert max(lens) == c["tmax"], case
    w = gru_weights(c["D"], c["H"], c["L"], seed)
    xs = [R.features(T, 1, c["D"], seed + 1 + i)[:, 0, :] - 0.2 for i, T in enumerate(lens)]
    cw = np.random.default_rng(seed + 99).standard_normal(sum(lens)).astype(np.float32)
    return dict(w=w, xs=xs, cw=cw, off=np.concatenate([[0], np.cumsum(lens)]).astype(int))


def yardstick_hook(case, mode, grads):
    """The matmul hook of a yardstick oracle (the products the library takes differently from a plain fp32 BLAS product; the test's
    docstring restates them from the source)."""
    step = CASES[case].get("step_path", False)
    if mode == "fp32" and grads:      # the dX GEMM's one accumulator chain over 3H columns per direction (torch_port.mm_chain)
        return lambda a, w, site: torch_port.LinearChainDx.apply(a, w) if site == "ih" else a @ w.t()
    if mode == "x3" and step:         # step path: every product and both backward products of each in bf16x3
        return lambda a, w, site: torch_port.Linear3.apply(a, w, False)
    if mode == "x3":                  # persistent path: projection, dX, dW_ih and dW_hh in bf16x3; recurrence and dGh . W_hh in fp32
        return lambda a, w, site: torch_port.Linear3.apply(a, w, False) if site == "ih" else torch_port.LinearDw3.apply(a, w)
    return None


def run_oracle(case, mode, grads, hook=None, gate_math=None):
    """bigru_stack_ref + head + the gradients of sum(scores * cw) in float64 (mode "f64") or float32; {name: float64 array}: h<l> (R, 2H),
    scores (R,), dx (R, D), the state_dict names."""
    inp = inputs(case)
    dt = F64 if mode == "f64" else torch.float32
    if gate_math is None:
        gate_math = "exact" if mode == "f64" or CASES[case].get("step_path", False) else "rcp_form"
    p = {k: torch.from_numpy(v).to(dt).requires_grad_(grads) for k, v in inp["w"].items()}
    xs = [torch.from_numpy(x).to(dt).requires_grad_(grads) for x in inp["xs"]]
    sig = torch_port.GATE_MATH[gate_math][0]
    with torch.set_grad_enabled(grads):
        layers = torch_port.bigru_stack_ref(xs, {k[4:]: v for k, v in p.items() if k.startswith("rnn.")}, gate_math=gate_math, matmul=hook)
        scores = sig(torch.cat(layers[-1]) @ p["out.0.weight"].t() + p["out.0.bias"])[:, 0]
        out = {f"h{l}": torch.cat(v) for l, v in enumerate(layers)}
        out["scores"] = scores
        if grads:
            names = list(p)
            g = torch.autograd.grad((scores * torch.from_numpy(inp["cw"]).to(dt)).sum(), xs + [p[n] for n in names])
            out["dx"] = torch.cat(g[:len(xs)])
            out.update(zip(names, g[len(xs):]))
    return {k: v.detach().to(F64).numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def oracle(case, mode, grads):
    """mode "f64": float64, exact gate functions (the reference); "fp32": float32 with the gate formulas of the path the case runs on
    (the yardstick); "x3": the fp32 yardstick with the bf16x3 products where the library runs them.  Cached; never modified."""
    return run_oracle(case, mode, grads, yardstick_hook(case, mode, grads))


def refs(case, precision, grads):
    """(float64 reference, yardstick oracle).  The float64 and plain fp32 runs of a case are shared by all its tests (gradients included
    unless the case is forward-only); bf16x6 is judged by the plain fp32 yardstick."""
    full = not CASES[case].get("forward_only", False)
    return oracle(case, "f64", full), (oracle(case, "x3", grads) if precision == "bf16x3" else oracle(case, "fp32", full))


# ------------------------------------------------------------------------------------------------ slices and the gate
def slices(case, grads):
    """[(kind, name, key in the judged dict, key in the oracle dicts, index, relative)] of a case.  Case h: scores of every video in both
    modes, dx of H_DX_VIDEOS, every parameter gradient."""
    c, off = CASES[case], inputs(case)["off"]
    H, lens = c["H"], c["lens"]
    rows = lambda v: slice(off[v], off[v + 1])
    sl = []
    for mode in ("", "train_") if grads else ("",):
        for l in range(c["L"]) if case != "h" else ():
            for v in range(len(lens)):
                for d, dn in enumerate(("fwd", "rev")):
                    sl.append((f"hidden_l{l}", f"{mode}h{l}[video {v}, T={lens[v]}, {dn}]", f"{mode}h{l}", f"h{l}",
                               (rows(v), slice(d * H, (d + 1) * H)), False))
        for v in range(len(lens)):
            sl.append(("scores", f"{mode}scores[video {v}, T={lens[v]}]", f"{mode}scores", "scores", (rows(v),), False))
    if grads:
        for v in (range(len(lens)) if case != "h" else H_DX_VIDEOS):
            sl.append(("dx", f"dx[video {v}, T={lens[v]}]", "dx", "dx", (rows(v),), True))
        for l in range(c["L"]):
            for suf in ("", "_reverse"):
                for t, kind in GRU_TENSORS:
                    for q, gate in enumerate("rzn"):
                        k = f"rnn.{t}_l{l}{suf}"
                        sl.append((kind, f"d{k}[{gate}]", k, k, (slice(q * H, (q + 1) * H),), True))
        for k in ("out.0.weight", "out.0.bias"):
            sl.append(("dhead", f"d{k}", k, k, (Ellipsis,), True))
    return sl


def judge(tag, case, got, ref, yard, grads, quiet=False):
    """Every slice of the case against float64: error of `got` <= FACTOR x the yardstick of the slice's kind (the largest
    |yard - ref| over the case's slices of that kind, floored at 2 fp32 ulps of the slice's largest reference magnitude).  Records
    yardsticks and worst ratios in REPORT; returns (record, [what is over the gate])."""
    rows, ys = [], {}
    for kind, name, gk, rk, idx, rel in slices(case, grads):
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
    rec = dict(case=tag, checks=len(rows), yardstick=ys, worst_ratio={k: v[0] for k, v in worst.items()},
               worst_slice={k: v[1] for k, v in worst.items()})
    REPORT.append(rec)
    if not quiet:
        print(f"\nGRU-F64 {tag}: {len(rows)} checks; yardsticks " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(ys.items())))
        print(f"GRU-F64 {tag}: worst err / yardstick " + ", ".join(f"{k} {v[0]:.2f} ({v[1]})" for k, v in sorted(worst.items())))
    return rec, bad


def assert_judged(tag, case, got, ref, yard, grads):
    rec, bad = judge(tag, case, got, ref, yard, grads)
    assert not bad, f"{tag}: {len(bad)} of {rec['checks']} over the gate: " + "; ".join(bad[:12])
