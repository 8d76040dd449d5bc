"""Shared by tests/test_gpu_sumgan_lstm_f64.py (SumGAN's one-direction LSTM layer and step-wise decoder kernels against float64) and
tests/test_sumgan_lstm_f64_host.py (the same gates on the CPU, a hand-written fp32 BPTT and planted errors standing in for the kernels):
the cases with the path each must reach, their inputs, the float64 reference and the fp32 / bf16x3 yardstick oracles
(oracle/torch_port.lstm_stack_ref, dlstm_ref), the slices, the gate and the stand-in.  Nothing here needs a GPU or the library."""
import functools

import numpy as np
import torch

from oracle import torch_port

ULP = 2.0 ** -24
FACTOR = 4.0
F64 = torch.float64
F32 = torch.float32
REPORT = []
GV_MAXB = 8                                      # csrc/lstm.hip: at most this many sequences take the mat-vec step kernels
PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
PARAM_KIND = dict(weight_ih="dweight_ih", weight_hh="dweight_hh", bias_ih="dbias", bias_hh="dbias")

_LENS_9 = [10, 1, 2, 7, 10, 4, 8, 3, 6]
_LENS_33 = [20, 1, 2] + [(7 * i) % 20 + 1 for i in range(30)]
LAYER_CASES = {
    "La": dict(H=40, In=24, L=1, lens=[7, 1, 2, 5, 7], state=True, tmax=7),
    "Lb": dict(H=104, In=32, L=1, lens=[9, 1, 2, 6, 9, 4, 7, 3], state=False, tmax=9),
    "Lc": dict(H=1060, In=64, L=1, lens=[12, 1, 5], state=True, tmax=12),
    "Ld": dict(H=40, In=24, L=1, lens=_LENS_9, state=True, tmax=10),
    "Le": dict(H=100, In=48, L=2, lens=_LENS_33, state=True, tmax=20),
    "Lf": dict(H=1028, In=64, L=1, lens=[6, 1, 2, 4, 6, 3, 5, 2, 4], state=True, tmax=6),
    "Lg": dict(H=256, In=64, L=1, lens=[160, 1, 2] + [160 - 10 * (i % 7) for i in range(63)], state=False, tmax=160),
}
DECODER_CASES = {
    "Da": dict(H=40, L=2, lens=[9, 1, 2, 9], tmax=9),
    "Db": dict(H=104, L=1, lens=[9, 1, 2, 6, 9, 4, 7, 3], tmax=9),
    "Dc": dict(H=1060, L=2, lens=[10, 4], tmax=10),
    "Dd": dict(H=40, L=3, lens=_LENS_9, tmax=10),
    "De1": dict(H=100, L=1, lens=_LENS_33, tmax=20),
    "De2": dict(H=100, L=2, lens=_LENS_33, tmax=20),
    "Df": dict(H=1028, L=2, lens=[6, 1, 2, 4, 6, 3, 5, 2, 4], tmax=6),
}
SEED = {c: 9100 + 100 * i for i, c in enumerate(sorted(LAYER_CASES) + sorted(DECODER_CASES))}


# ------------------------------------------------------------------------------------------------ the plan, restated
# csrc/lstm.hip: few_sequences / GV_MAXB, tgemv_geom, lstm_carve(nd = 1) / dec_carve, the grids of fwd_matvec / fwd_chain / bwd_matvec /
# bwd_chain and of the decoder's launches, the k loops of the step kernels; csrc/sumk_internal.h: gemm_tiles.
def tgemv_geom(H):
    strips, H4 = (H + 255) // 256, 4 * H
    want = min(max(1, 2048 // strips), max(1, H4 // 32), 128)
    rps = ((H4 + want - 1) // want + 3) // 4 * 4
    n = (H4 + rps - 1) // rps
    return dict(strips=strips, last_strip=H - (strips - 1) * 256, n_ksplit=n, rows_per_split=rps, last_split=H4 - (n - 1) * rps)


def plan(H, n_seq, n_rows=None, In=None):
    """The path of a one-direction layer (In, n_rows given: with its input projection) or of a decoder layer of this shape."""
    few = n_seq <= GV_MAXB
    p = dict(few=few, n_mtiles=(n_seq + 31) // 32, last_mtile=n_seq - ((n_seq + 31) // 32 - 1) * 32)
    if few:
        g = tgemv_geom(H)
        p.update(g)
        p["idle_lanes"] = H // 4 < 64                                      # lstm_gemv_step_kernel: lane l loads k = 4 l + 256 u
        p["k_chunk2_lanes"] = max(0, (H - 1024 + 3) // 4)                  # lanes live in the second 1024-wide k chunk
        # lstm_cellbwd_kernel: group grp = 0..3 walks s = grp, grp + 16, ... four at a time while s + 12 < n_ksplit, then one at a time
        p["stride16_runs"] = max((max(0, g["n_ksplit"] - 12 - grp) + 15) // 16 for grp in range(4))
        p["tail_runs"] = any((g["n_ksplit"] - grp) > 16 * ((max(0, g["n_ksplit"] - 12 - grp) + 15) // 16) for grp in range(4))
    else:
        p.update(n_ublk=(H + 7) // 8, last_ublk=H - ((H + 7) // 8 - 1) * 8, n_jblk=(H + 31) // 32, last_jblk=H - ((H + 31) // 32 - 1) * 32)
        p["k_tail_chunks"] = ((H + 7) // 8) % 32                           # lstm_step_kernel: 8-wide k chunks, 32 per trip of the four waves
        p["k_tail_chunks_dec"] = ((H + 7) // 8) % 16                       # lstm_dec_step_kernel: 16 per trip
    if In is not None:
        tiles128 = ((n_rows + 127) // 128) * ((4 * H + 127) // 128)
        p["proj_tile"] = 128 if tiles128 >= 512 else 64
    return p


REGIME = {
    "La": dict(few=True, idle_lanes=True, strips=1, last_strip=40, n_ksplit=5, stride16_runs=0, tail_runs=True, k_chunk2_lanes=0, proj_tile=64),
    "Lb": dict(few=True, n_ksplit=13, stride16_runs=1, tail_runs=True, strips=1, proj_tile=64),
    "Lc": dict(few=True, k_chunk2_lanes=9, strips=5, last_strip=36, n_ksplit=118, last_split=28, rows_per_split=36),
    "Ld": dict(few=False, n_mtiles=1, n_ublk=5, last_ublk=8, n_jblk=2, last_jblk=8),
    "Le": dict(few=False, n_mtiles=2, last_mtile=1, n_ublk=13, last_ublk=4, n_jblk=4, last_jblk=4, proj_tile=64),
    "Lf": dict(few=False, n_mtiles=1, k_tail_chunks=1, n_ublk=129, last_ublk=4),
    "Lg": dict(few=False, n_mtiles=3, last_mtile=2, proj_tile=128, n_ublk=32, n_jblk=8),
    "Da": dict(few=True, idle_lanes=True, n_ksplit=5, strips=1),
    "Db": dict(few=True, n_ksplit=13, stride16_runs=1),
    "Dc": dict(few=True, k_chunk2_lanes=9, strips=5, last_strip=36, n_ksplit=118, last_split=28),
    "Dd": dict(few=False, n_mtiles=1, n_ublk=5, n_jblk=2, last_jblk=8),
    "De1": dict(few=False, n_mtiles=2, last_mtile=1, n_ublk=13, last_ublk=4, n_jblk=4, last_jblk=4),
    "De2": dict(few=False, n_mtiles=2, last_mtile=1, n_ublk=13, last_ublk=4, n_jblk=4, last_jblk=4),
    "Df": dict(few=False, n_mtiles=1, k_tail_chunks_dec=1, n_ublk=129),
}


def check_regime(case):
    """The path the case is named for, from the plan restated above; also the batch rules of the issue's case table."""
    layer = case in LAYER_CASES
    c = LAYER_CASES[case] if layer else DECODER_CASES[case]
    lens = c["lens"]
    got = plan(c["H"], len(lens), sum(lens), c["In"]) if layer else plan(c["H"], len(lens))
    want = REGIME[case]
    assert {k: got.get(k) for k in want} == want, (case, got, want)
    assert max(lens) == c["tmax"] and (c["tmax"] <= 160), case
    if len(lens) > 3:
        assert 1 in lens and 2 in lens and len(set(lens)) < len(lens), case
    if case == "Lb":
        assert len(lens) == GV_MAXB and not c["state"]
    if case in ("Ld", "Dd"):
        assert len(lens) == GV_MAXB + 1
    if case == "Lg":
        assert sum(lens) >= 8065 and len(lens) == 66
    if case == "Le":                                                    # layer 1 (In = H) runs the same step path
        assert plan(c["H"], len(lens), sum(lens), c["H"])["few"] == got["few"]
    if case == "Dd":
        assert c["L"] == 3                                              # a middle layer: neither layer 0 nor the top
    return got


# ------------------------------------------------------------------------------------------------ inputs
def _randn(shape, seed, scale=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _lstm_init(In, H, L, seed):
    """Stock nn.LSTM initialisation (uniform +- 1 / sqrt(H)), seeded without touching the global generator."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return {k: v.detach().clone() for k, v in torch.nn.LSTM(In, H, num_layers=L).state_dict().items()}


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(int)


@functools.lru_cache(maxsize=None)
def layer_inputs(case):
    """Weights, one feature block per video (its own seed, scaled 0.5), h0 (0.3) / c0 (0.4) and the fixed loss weights on the top layer's
    rows, h_n and c_n.  fp32 torch tensors; never modified."""
    c, seed = LAYER_CASES[case], SEED[case]
    H, L, lens, B = c["H"], c["L"], c["lens"], len(c["lens"])
    return dict(w=_lstm_init(c["In"], H, L, seed), xs=[_randn((T, c["In"]), seed + 1 + i, 0.5) for i, T in enumerate(lens)],
                h0=_randn((L, B, H), seed + 200, 0.3) if c["state"] else None, c0=_randn((L, B, H), seed + 201, 0.4) if c["state"] else None,
                cw_out=_randn((sum(lens), H), seed + 300), cw_h=_randn((L, B, H), seed + 400), cw_c=_randn((L, B, H), seed + 401),
                off=_offsets(lens))


@functools.lru_cache(maxsize=None)
def decoder_inputs(case):
    c, seed = DECODER_CASES[case], SEED[case]
    H, L, lens, B = c["H"], c["L"], c["lens"], len(c["lens"])
    return dict(w=_lstm_init(H, H, L, seed), h0=_randn((L, B, H), seed + 200, 0.3), c0=_randn((L, B, H), seed + 201, 0.4),
                cw=_randn((sum(lens), H), seed + 300), off=_offsets(lens))


# ------------------------------------------------------------------------------------------------ oracles
def yardstick_hook(mode, decoder=False):
    """The products the kernels take differently from a plain fp32 product (read from csrc/lstm.hip):
    layer, fp32   sumk_lstm_layer_backward's dX GEMM sums K = 4H gate columns in one MFMA accumulator chain (LinearChainDx; the weight
                  gradients are split-K: many short chains, a plain product);
    layer, x3     the input projection with its dx and dW_ih in bf16x3 (Linear3), dW_hh in bf16x3 (LinearDw3: dir_grad_tail passes the
                  layer's precision to both weight-gradient products); the recurrent products and the BPTT's dG . W_hh stay fp32;
    decoder       every product fp32 on short chains (dir_grad_tail at its default precision): plain products, in the kernels' order."""
    if decoder:
        return lambda a, w, site: a @ w.t()
    if mode == "x3":
        return lambda a, w, site: torch_port.Linear3.apply(a, w, False) if site == "ih" else torch_port.LinearDw3.apply(a, w)
    return lambda a, w, site: torch_port.LinearChainDx.apply(a, w) if site == "ih" else a @ w.t()


def _np(d):
    return {k: v.detach().to(F64).numpy() for k, v in d.items()}


def run_layer_oracle(case, mode, hook=None, gate_math=None):
    """lstm_stack_ref and the gradients of sum(out_top cw_out) + sum(h_n cw_h) + sum(c_n cw_c), in float64 (mode "f64") or float32.
    {name: float64 array}: h<l> (R, H), hn, cn (L, B, H), dx (R, In), dh0 / dc0 (L, B, H) with an initial state, the state_dict names."""
    c, inp = LAYER_CASES[case], layer_inputs(case)
    dt = F64 if mode == "f64" else F32
    leaf = lambda t: t.detach().to(dt, copy=True).requires_grad_(True)           # (a copy: the cached inputs stay plain tensors)
    p = {k: leaf(v) for k, v in inp["w"].items()}
    xs = [leaf(x) for x in inp["xs"]]
    h0, c0 = (leaf(inp["h0"]), leaf(inp["c0"])) if c["state"] else (None, None)
    lo = []
    outs, (hn, cn) = torch_port.lstm_stack_ref(xs, p, h0, c0, gate_math=gate_math or ("exact" if mode == "f64" else "rcp_sigmoid"),
                                               matmul=hook, layer_outs=lo)
    loss = (torch.cat(outs) * inp["cw_out"].to(dt)).sum() + (hn * inp["cw_h"].to(dt)).sum() + (cn * inp["cw_c"].to(dt)).sum()
    names = list(p)
    g = torch.autograd.grad(loss, xs + [p[n] for n in names] + ([h0, c0] if c["state"] else []))
    out = {f"h{l}": torch.cat(v) for l, v in enumerate(lo)}
    out.update(hn=hn, cn=cn, dx=torch.cat(g[:len(xs)]))
    out.update(zip(names, g[len(xs):len(xs) + len(names)]))
    if c["state"]:
        out.update(dh0=g[-2], dc0=g[-1])
    return _np(out)


def run_decoder_oracle(case, state, mode, hook=None, gate_math=None):
    """dlstm_ref(recons=None) and the gradients of sum(out cw); state False: zero h0 / c0 (their gradients exist all the same).
    {name: float64 array}: out (R, H), dh0, dc0 (L, B, H), the state_dict names."""
    c, inp = DECODER_CASES[case], decoder_inputs(case)
    dt = F64 if mode == "f64" else F32
    leaf = lambda t: t.detach().to(dt, copy=True).requires_grad_(True)           # (a copy: the cached inputs stay plain tensors)
    p = {k: leaf(v) for k, v in inp["w"].items()}
    h0, c0 = leaf(inp["h0"] if state else torch.zeros_like(inp["h0"])), leaf(inp["c0"] if state else torch.zeros_like(inp["c0"]))
    outs = torch_port.dlstm_ref(p, None, c["lens"], h0, c0, gate_math=gate_math or ("exact" if mode == "f64" else "rcp_sigmoid"), matmul=hook)
    names = list(p)
    g = torch.autograd.grad((torch.cat(outs) * inp["cw"].to(dt)).sum(), [h0, c0] + [p[n] for n in names])
    out = dict(out=torch.cat(outs), dh0=g[0], dc0=g[1])
    out.update(zip(names, g[2:]))
    return _np(out)


@functools.lru_cache(maxsize=None)
def layer_oracle(case, mode):
    """mode "f64": float64, exact gate functions (the reference); "fp32": float32 with the step kernels' gate formulas (sigmoidf_ =
    1 / (1 + expf(-v)), the library's tanhf: GATE_MATH["rcp_sigmoid"]) and the dX chain; "x3": that with the bf16x3 products.  Cached; never
    modified."""
    return run_layer_oracle(case, mode, None if mode == "f64" else yardstick_hook(mode))


@functools.lru_cache(maxsize=None)
def decoder_oracle(case, state, mode):
    return run_decoder_oracle(case, state, mode, None if mode == "f64" else yardstick_hook(mode, decoder=True))


def layer_refs(case, precision):
    """(float64 reference, yardstick).  bf16x6 is advertised as fp32-grade: the plain fp32 yardstick."""
    return layer_oracle(case, "f64"), layer_oracle(case, "x3" if precision == "bf16x3" else "fp32")


def decoder_refs(case, state):
    return decoder_oracle(case, state, "f64"), decoder_oracle(case, state, "fp32")


# ------------------------------------------------------------------------------------------------ slices and the gate
def _param_slices(prefix, H, L):
    sl = []
    for l in range(L):
        for t in PARAMS:
            for q, gate in enumerate("ifgo"):
                k = f"{t}_l{l}"
                sl.append((PARAM_KIND[t], f"d{k}[{gate}]", prefix + k, k, (slice(q * H, (q + 1) * H),), True))
    return sl


def layer_slices(case, infer=True, train=True, want_d0=True):
    """[(kind, name, key in the judged dict, key in the oracle dicts, index, relative)].  infer: the no_grad run (hidden states of every
    layer, h_n, c_n); train: the training run (top layer's rows, h_n, c_n, every gradient; dh0 / dc0 with an initial state and want_d0)."""
    c, off = LAYER_CASES[case], layer_inputs(case)["off"]
    H, L, lens = c["H"], c["L"], c["lens"]
    rows = lambda v: slice(off[v], off[v + 1])
    sl = []
    for mode, layers in (("", range(L)),) * infer + (("train_", (L - 1,)),) * train:
        for l in layers:
            for v, T in enumerate(lens):
                sl.append((f"hidden_l{l}", f"{mode}h{l}[video {v}, T={T}]", f"{mode}h{l}", f"h{l}", (rows(v),), False))
        for l in range(L):
            for v in range(len(lens)):
                sl.append(("h_n", f"{mode}h_n[layer {l}, video {v}]", f"{mode}hn", "hn", (l, v), False))
                sl.append(("c_n", f"{mode}c_n[layer {l}, video {v}]", f"{mode}cn", "cn", (l, v), False))
    if train:
        for v, T in enumerate(lens):
            sl.append(("dx", f"dx[video {v}, T={T}]", "dx", "dx", (rows(v),), True))
        if c["state"] and want_d0:
            for l in range(L):
                for v in range(len(lens)):
                    sl.append(("dh0", f"dh0[layer {l}, video {v}]", "dh0", "dh0", (l, v), True))
                    sl.append(("dc0", f"dc0[layer {l}, video {v}]", "dc0", "dc0", (l, v), True))
        sl += _param_slices("", H, L)
    return sl


def decoder_slices(case, want_d0=True):
    c, off = DECODER_CASES[case], decoder_inputs(case)["off"]
    sl = [("out", f"out[video {v}, T={T}]", "out", "out", (slice(off[v], off[v + 1]),), False) for v, T in enumerate(c["lens"])]
    if want_d0:
        for l in range(c["L"]):
            for v in range(len(c["lens"])):
                sl.append(("dh0", f"dh0[layer {l}, video {v}]", "dh0", "dh0", (l, v), True))
                sl.append(("dc0", f"dc0[layer {l}, video {v}]", "dc0", "dc0", (l, v), True))
    return sl + _param_slices("", c["H"], c["L"])


def assert_reference_nowhere_zero(tag, slices, ref):
    """On the float64 run: no slice of the case is identically zero (the inputs keep every gate away from saturation)."""
    zero = [name for _, name, _, rk, idx, _ in slices if not np.abs(ref[rk][idx]).max() > 0]
    assert not zero, (tag, zero[:8])


def judge(tag, slices, got, ref, yard, quiet=False):
    """Every slice against float64: error of `got` <= FACTOR x the yardstick of the slice's kind (the largest |yard - ref| over the case's
    slices of that kind, floored at 2 fp32 ulps = 2^-23 of the slice's largest reference magnitude).  Forward slices: largest absolute
    error; gradient slices: that divided by the slice's largest reference magnitude.  No slice is skipped: one whose reference is
    identically zero must come out exactly zero.  Records yardsticks and worst ratios in REPORT; returns (record, [what is over the gate])."""
    rows, ys, bad = [], {}, []
    for kind, name, gk, rk, idx, rel in slices:
        r = ref[rk][idx]
        assert got[gk].shape == ref[rk].shape, (tag, name, got[gk].shape, ref[rk].shape)
        scale = float(np.abs(r).max())
        if not scale > 0:
            if not float(np.abs(got[gk][idx]).max()) == 0.0:
                bad.append(f"{name}: the reference is zero, the value is not")
            continue
        den = scale if rel else 1.0
        ey = float(np.abs(yard[rk][idx] - r).max()) / den
        eh = float(np.abs(got[gk][idx] - r).max()) / den                  # NaN / inf: fails `eh <= gate` below
        rows.append((kind, name, eh, 2 * ULP * (1.0 if rel else scale)))
        ys[kind] = max(ys.get(kind, 0.0), ey)
    worst = {}
    for kind, name, eh, floor in rows:
        y = max(ys[kind], floor)
        ratio = eh / y
        if not ratio <= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (ratio, name)
        if not eh <= FACTOR * y:
            bad.append(f"{name}: {eh:.3e} > {FACTOR:g} x {y:.3e}")
    rec = dict(case=tag, checks=len(slices), yardstick=ys, worst_ratio={k: v[0] for k, v in worst.items()},
               worst_slice={k: v[1] for k, v in worst.items()})
    REPORT.append(rec)
    if not quiet:
        print(f"\nSUMGAN-LSTM-F64 {tag}: {len(slices)} checks; yardsticks " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(ys.items())))
        print(f"SUMGAN-LSTM-F64 {tag}: worst err / yardstick " + ", ".join(f"{k} {v[0]:.2f} ({v[1]})" for k, v in sorted(worst.items())))
    return rec, bad


def assert_judged(tag, slices, got, ref, yard):
    rec, bad = judge(tag, slices, got, ref, yard)
    assert not bad, f"{tag}: {len(bad)} of {rec['checks']} over the gate: " + "; ".join(bad[:12])
    return rec


# ------------------------------------------------------------------------------------------------ the stand-in
# A hand-written fp32 forward + BPTT in the kernels' own structure (saved gates, cell states and h_{t-1}; dG per row; the running dc; the
# extra step t = -1 for dh0 / dc0; the weight gradients as products over the packed rows afterwards), with torch.sigmoid / torch.tanh and
# plain products: an fp32 realisation that is neither the yardstick nor autograd.  `mutant` plants one error (the host test names them).
def _cell_fwd(pre, cprev):
    i, f, g, o = pre.chunk(4, dim=-1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * cprev + i * g
    return o * torch.tanh(c), c, torch.cat([i, f, g, o], dim=-1)


def _cell_bwd(dh, dc_in, gates, c, cprev):
    i, f, g, o = gates.chunk(4, dim=-1)
    tc = torch.tanh(c)
    dc = dc_in + dh * o * (1.0 - tc * tc)
    dG = torch.cat([dc * g * i * (1.0 - i), dc * cprev * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)], dim=-1)
    return dG, dc


def standin_layer(case, mutant=None, video=0, block=1):
    """The layer stack of a case; keys as the GPU test's run: h<l>, hn, cn (and train_ copies), dx, dh0, dc0, the state_dict names.
    mutant (acts on layer 0, on `video`): "dwhh_block" gate block `block` of dW_hh times 1 + 1e-4; "dwih_last_step" the video's last step
    missing from dW_ih; "dc0_no_forget" dc0 taken before the final multiplication by the forget gate; "h0_ignored" the video's first step
    multiplies W_hh by zeros; "dh_last_early" the video's dh_last added one step before its last."""
    c, inp = LAYER_CASES[case], layer_inputs(case)
    H, L, lens, B, off = c["H"], c["L"], c["lens"], len(c["lens"]), inp["off"]
    T, r0 = torch.tensor(lens), torch.from_numpy(off[:-1])
    R = int(off[-1])
    zeros = lambda *s: torch.zeros(*s, dtype=F32)
    W = lambda l: [inp["w"][f"{t}_l{l}"] for t in PARAMS]
    acts, saves, hn, cn = [torch.cat(inp["xs"])], [], [], []
    for l in range(L):
        w_ih, w_hh, b_ih, b_hh = W(l)
        G = acts[-1] @ w_ih.t() + b_ih + b_hh
        h, call, hprev, gates = zeros(R, H), zeros(R, H), zeros(R, H), zeros(R, 4 * H)
        for t in range(c["tmax"]):
            b = (T > t).nonzero()[:, 0]
            r = r0[b] + t
            hp = h[r - 1] if t > 0 else (inp["h0"][l][b] if c["state"] else zeros(len(b), H))
            cp = call[r - 1] if t > 0 else (inp["c0"][l][b] if c["state"] else zeros(len(b), H))
            a2 = hp
            if mutant == "h0_ignored" and l == 0 and t == 0:
                a2 = hp * (b != video)[:, None]
            h[r], call[r], gates[r] = _cell_fwd(G[r] + a2 @ w_hh.t(), cp)
            hprev[r] = hp
        last = r0 + T - 1
        hn.append(h[last]); cn.append(call[last])
        acts.append(h); saves.append((gates, call, hprev))
    out = {f"h{l}": acts[l + 1] for l in range(L)}
    out.update(hn=torch.stack(hn), cn=torch.stack(cn))
    dext, dh0s, dc0s = inp["cw_out"], [], []
    for l in range(L - 1, -1, -1):
        w_ih, w_hh, b_ih, b_hh = W(l)
        gates, call, hprev = saves[l]
        dG, dcs, dc_raw = zeros(R, 4 * H), zeros(B, H), zeros(B, H)
        at = T - 1                                                    # the step that receives dh_last
        if mutant == "dh_last_early" and l == 0:
            assert lens[video] >= 2
            at = at.clone(); at[video] -= 1
        for t in range(c["tmax"] - 1, -1, -1):
            b = (T > t).nonzero()[:, 0]
            r = r0[b] + t
            more = T[b] > t + 1
            dh = dext[r].clone()
            dh[more] += dG[r[more] + 1] @ w_hh
            hit = at[b] == t
            dh[hit] += inp["cw_h"][l][b[hit]]
            dc_in = torch.where(more[:, None], dcs[b], inp["cw_c"][l][b])
            cp = call[r - 1] if t > 0 else (inp["c0"][l][b] if c["state"] else zeros(len(b), H))
            dG[r], dc = _cell_bwd(dh, dc_in, gates[r], call[r], cp)
            dcs[b], dc_raw[b] = dc * gates[r][:, H:2 * H], dc
        dh0s.append(dG[r0] @ w_hh)                                    # the extra step t = -1
        dc0s.append(dc_raw if (mutant == "dc0_no_forget" and l == 0) else dcs)
        dGi = dG
        if mutant == "dwih_last_step" and l == 0:
            dGi = dG.clone(); dGi[off[video + 1] - 1] = 0.0
        gw = [dGi.t() @ acts[l], dG.t() @ hprev, dG.sum(0), dG.sum(0)]
        if mutant == "dwhh_block" and l == 0:
            gw[1][block * H:(block + 1) * H] *= 1.0 + 1e-4
        out.update({f"{t}_l{l}": g for t, g in zip(PARAMS, gw)})
        dext = dG @ w_ih
    out["dx"] = dext
    if c["state"]:
        out.update(dh0=torch.stack(dh0s[::-1]), dc0=torch.stack(dc0s[::-1]))
    out = _np(out)
    out.update({f"train_{k}": out[k] for k in [f"h{L - 1}", "hn", "cn"]})
    return out


def standin_decoder(case, state, mutant=None, feed=None):
    """The decoder of a case; keys out, dh0, dc0, the state_dict names.  mutant: "feed_same_step" layer 0 reads `feed` (R, H: a clean
    run's top-layer rows) at its OWN row, h_top[t], where it should read h_top[t - 1] (zeros at t = 0); "top_misses_wih0" the top layer's
    backward lacks the term dG_0[t + 1] . W_ih_0 (its output is layer 0's input at the next step)."""
    c, inp = DECODER_CASES[case], decoder_inputs(case)
    H, L, lens, B, off = c["H"], c["L"], c["lens"], len(c["lens"]), inp["off"]
    T, r0 = torch.tensor(lens), torch.from_numpy(off[:-1])
    R, top = int(off[-1]), L - 1
    zeros = lambda *s: torch.zeros(*s, dtype=F32)
    W = [[inp["w"][f"{t}_l{l}"] for t in PARAMS] for l in range(L)]
    h0 = inp["h0"] if state else zeros(L, B, H)
    c0 = inp["c0"] if state else zeros(L, B, H)
    hs, call, hprev, xin = ([zeros(R, H) for _ in range(L)] for _ in range(4))
    gates = [zeros(R, 4 * H) for _ in range(L)]
    for t in range(c["tmax"]):
        b = (T > t).nonzero()[:, 0]
        r = r0[b] + t
        for l in range(L):
            w_ih, w_hh, b_ih, b_hh = W[l]
            a1 = (hs[top][r - 1] if t > 0 else zeros(len(b), H)) if l == 0 else hs[l - 1][r]
            if mutant == "feed_same_step" and l == 0:
                a1 = feed[r]
            a2 = hs[l][r - 1] if t > 0 else h0[l][b]
            cp = call[l][r - 1] if t > 0 else c0[l][b]
            hs[l][r], call[l][r], gates[l][r] = _cell_fwd((b_ih + b_hh) + (a1 @ w_ih.t() + a2 @ w_hh.t()), cp)
            xin[l][r], hprev[l][r] = a1, a2
    dG, dcs = [zeros(R, 4 * H) for _ in range(L)], [zeros(B, H) for _ in range(L)]
    for t in range(c["tmax"] - 1, -1, -1):
        b = (T > t).nonzero()[:, 0]
        r = r0[b] + t
        more = T[b] > t + 1
        for l in range(top, -1, -1):
            dh = inp["cw"][r].clone() if l == top else zeros(len(b), H)
            dh[more] += dG[l][r[more] + 1] @ W[l][1]
            if l == top:
                if mutant != "top_misses_wih0":
                    dh[more] += dG[0][r[more] + 1] @ W[0][0]
            else:
                dh += dG[l + 1][r] @ W[l + 1][0]
            cp = call[l][r - 1] if t > 0 else c0[l][b]
            dG[l][r], dc = _cell_bwd(dh, dcs[l][b] * more[:, None], gates[l][r], call[l][r], cp)
            dcs[l][b] = dc * gates[l][r][:, H:2 * H]
    out = dict(out=hs[top], dh0=torch.stack([dG[l][r0] @ W[l][1] for l in range(L)]), dc0=torch.stack(dcs))
    for l in range(L):
        out.update({f"{t}_l{l}": g for t, g in zip(PARAMS, (dG[l].t() @ xin[l], dG[l].t() @ hprev[l], dG[l].sum(0), dG[l].sum(0)))})
    return _np(out)
