"""Shared by tests/test_vasnet_bf16_host.py (CPU) and tests/test_gpu_vasnet_bf16_f64.py (GPU): the float64 reference of VASNet's
mixed-precision training step (precision="bf16"), its yardstick, the metric, the gates and the dispatch restated from the source.
Importable without a GPU.

REFERENCE (E64).  oracle/torch_port.vasnet_scores(..., bf16_products=True) on float64 tensors, one video at a time, with plain torch ops
on whatever device the inputs live on: every operand of every matrix product is rounded fp32 -> bf16 (round to nearest even), forward and
backward; everything else -- accumulation, softmax, LayerNorm, residual, head -- is float64.  Dropout takes the deterministic masks of
recipes.vasnet_drop_masks(seed, p, lens, D), which index by the PACKED row.

ROUNDING POINTS the reference assumes, and where each was read in csrc/vasnet.hip (G.b16 = the bf16-source kernels of gemm_b16.hip):
  x, Wq/Wk/Wv/Wo/W1   forward_dense: cast_flat_b16 writes the six shadows (x16, w16) before the first GEMM
  Q, K, V             forward_dense stage 1: C16 = qkv16, C = nullptr -- only the bf16 form exists
  dropped alpha       vasnet_softmax_kernel: p16[j] = bf16(ad), ad = dropout(alpha) (fp32 alpha stays in E for the softmax backward)
  CTX                 attn_grouped stage 4: C16 = ctx16, C = nullptr
  Y1                  forward_dense stage 6: launch_ln_rows writes y116 only (Y0 = CTX Wo^T + x stays fp32: residual in the epilogue)
  dZ                  backward_dense 8': launch_ln_bwd<true> writes dZ16 (db1 = column sums of the fp32 dZ, before the rounding)
  dY0                 backward_dense 6': launch_ln_bwd<false> writes dY016; the fp32 dY0 exists only as dX's residual term ((b16 && !dx):
                      not at all)
  dCTX                backward_dense 5': C16 = dctx16, C = nullptr
  dLogits             vasnet_softmax_bwd_kernel<0>: s16[j] = bf16(alpha (dAlpha - dot) scale) -- the scale is applied BEFORE the rounding,
                      as the port's Bmm16 backward sees d(e * scale)
  dQ, dK, dV          backward_dense 4' / 2': C16 = dQKV16, C = nullptr; dW_qkv = dQKV16^T x16 and dX += dQKV16 W16 read that form
  Z (k1's output), the logits E, dAlpha, dY1 and dX are fp32 sums of bf16 products and are not rounded.
The port's _Linear16 / _Bmm16 round exactly these operands (a gradient is rounded where the product that consumes it reads it), so the
port needed no new rounding point -- only to run in float64 (its _r16 forced fp32).
The fused strips (t_max <= 320, csrc/attn_b16.hip) round at the same points (bf16 P / dS / CTX / dQ: test_gpu_attn_strip.py), and so do
the in-loop converting kernels of a small batch (use_b16 false; csrc/gemm_split.hip NS = 1: x1 = bf16(x) for both operands of every
product, the fp32 intermediates are rounded as they enter LDS) -- test_bf16_source_step_equals_the_plane_kernel_step finds the two
bit-identical in scores and dX.  One reference serves all three paths; no path has an emulation flag of its own.

YARDSTICK: a reference-only ensemble per case and per tensor.  E64 again with x and every parameter moved by one fp32 ulp in seeded random
directions (N_NUDGE seeds), and once with fp32 accumulation and fp32 row arithmetic (the port in float32).  Such a perturbation is far
below bf16 resolution; what it changes is on which side of a bf16 boundary some operands land -- the only thing that separates a correct
kernel from E64.  The yardstick of a tensor is the largest distance of any member to E64; it never sees the kernels.

METRIC: relative L2 per tensor -- the ten parameter gradients, dX, and the pre-sigmoid logits recovered from the scores -- and, for dX and
the logits, per video as well (a broken 47-frame video is not diluted by a 3000-frame neighbour).  Max-entry metrics are dominated by
single rounding flips and are not gated.

GATE: MULT x yardstick, floor 16 fp32 ulps (relative).  MULT = 4, the project's margin (test_gpu_vasnet_lengths.FP32_MULT)."""
import json
import os

import numpy as np
import torch

import recipes as R
import test_gpu_vasnet_lengths as L
from oracle import torch_port

MULT = 4.0
FLOOR = 16 * 2.0 ** -24
N_NUDGE = 3
MATS = ("K.weight", "Q.weight", "V.weight", "attention_head_projection.weight", "k1.weight")
MASKS = {"plain": {}, "noself": dict(ignore_self=True), "band64": dict(aperture=64)}
SEED, W_SEED = 777, 6

REPORT = []


def dump_report():
    path = os.environ.get("SUMK_BF16_LENGTHS_REPORT")    # optional: every error, yardstick and gate as JSON
    if path:
        short = lambda o: float(f"{o:.4g}") if isinstance(o, float) else {k: short(v) for k, v in o.items()} if isinstance(o, dict) else o
        with open(path, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(short(r), separators=(",", ":")) for r in REPORT) + "\n]\n")


# ------------------------------------------------------------------------------------------------ the dispatch, restated from the source
def _tiles128(M, N):
    return -(-M // 128) * -(-N // 128)                                              # gemm_tiles(M, N, 0)


def rowwise_small_tile(M, N):
    return 0 if _tiles128(M, N) >= 512 else 1                                      # csrc/vasnet.hip


def gemm_b16_ok(M, N, K, lda, ldb, kc_a, kc_b):                                    # csrc/sumk_internal.h
    lim = 1 << 31
    if lda % 8 or ldb % 8:
        return False
    if (K % 64 != 0 or (M + 128) * lda * 2 >= lim) if kc_a else (M % 8 != 0 or (K + 64) * lda * 2 >= lim):
        return False
    if (K % 64 != 0 or (N + 128) * ldb * 2 >= lim) if kc_b else (N % 8 != 0 or (K + 64) * ldb * 2 >= lim):
        return False
    return True


def gemm_b16_wide_bm(M, N):                                                        # csrc/sumk_internal.h
    tw = lambda bm: -(-M // bm) * -(-N // 256)
    t192, t256 = tw(192), tw(256)
    if t256 < 96 or N % 256 != 0:
        return 0
    return 192 if -(-t192 // 256) * 192 <= -(-t256 // 256) * 256 else 256


def use_b16(Rw, D, t_max):
    """csrc/vasnet.hip use_b16 for a training step in precision bf16 with SUMK_BF16_SRC unset."""
    ld16 = (t_max + 63) // 64 * 64
    if (t_max + 128) * ld16 * 2 >= 1 << 31:
        return False
    return (rowwise_small_tile(Rw, 3 * D) == 0 and rowwise_small_tile(Rw, D) == 0 and gemm_b16_ok(Rw, 3 * D, D, D, D, True, True)
            and gemm_b16_ok(Rw, D, D, D, D, True, False) and gemm_b16_ok(Rw, D, D, 3 * D, D, True, False)
            and gemm_b16_ok(3 * D, D, Rw, 3 * D, D, False, False))


def min_rows_b16(D):
    """The first R at which use_b16 holds for short videos (both row-wise problems on at least 512 tiles of 128 x 128)."""
    Rw = 1
    while not use_b16(Rw, D, 64):
        Rw += 1
    return Rw


def regime(lens, D):
    """What the bf16 training step runs for this batch: geometry() / use_b16 / attn_strip_ok / softmax_nr / to_b16 of csrc/vasnet.hip."""
    Rw, t_max = sum(lens), max(lens)
    b16 = use_b16(Rw, D, t_max)
    fused = b16 and 1 <= t_max <= 320 and D % 256 == 0 and D >= 256 and ((t_max + 64) * 3 * D + D) * 2 < 1 << 31      # attn_strip_ok
    return dict(R=Rw, n_seq=len(lens), t_max=t_max, b16=b16, attn_fused=fused, path="fused" if fused else "grouped" if b16 else "inloop",
                softmax_nr=4 if t_max <= 256 else 8 if t_max <= 512 else 16 if t_max <= 1024 else 0, ld16=(t_max + 63) // 64 * 64,
                bm_qkv=gemm_b16_wide_bm(Rw, 3 * D) if b16 else 0, bm_d=gemm_b16_wide_bm(Rw, D) if b16 else 0,
                tile128_fp32=Rw // len(lens) >= 1024)


# ------------------------------------------------------------------------------------------------ cases
def _filled(head, D, seed):
    return L._lens_fill(head, 150, 320, min_rows_b16(D), seed)


# id: (lens, D, expected regime entries, runs).  A run is (mask, dropout p, want_dx).
FULL = (("plain", 0.5, True), ("noself", 0.5, True), ("band64", 0.5, True), ("plain", 0.0, True), ("plain", 0.5, False))
CASES = {
    "fused_320": (_filled([320, 319, 257, 64, 47, 2], 1024, 1), 1024, dict(path="fused", t_max=320, softmax_nr=8), FULL),
    "grouped_321": (_filled([321, 320, 64, 2], 1024, 2), 1024, dict(path="grouped", t_max=321, softmax_nr=8, ld16=384), FULL),
    "grouped_512": (_filled([512, 511, 448], 1024, 3), 1024, dict(path="grouped", t_max=512, softmax_nr=8), FULL),
    "grouped_513": (_filled([513, 400, 2], 1024, 4), 1024, dict(path="grouped", t_max=513, softmax_nr=16), FULL),
    "grouped_1024": (_filled([1024, 1023, 700, 33], 1024, 5), 1024, dict(path="grouped", t_max=1024, softmax_nr=16), FULL),
    "stream_1025": (_filled([1025, 1024, 600, 3], 1024, 6), 1024, dict(path="grouped", t_max=1025, softmax_nr=0), FULL),
    "long_ragged": (_filled([3000, 1537, 1536, 70], 1024, 7), 1024, dict(path="grouped", softmax_nr=0, tile128_fp32=False), FULL),
    # (a lone long video: seconds only without the T x T dropout mask and with two masks)
    "lone_8101": ([8101], 1024, dict(path="grouped", n_seq=1, R=8101, softmax_nr=0),
                  (("plain", 0.0, True), ("noself", 0.0, True), ("plain", 0.0, False))),
    "d2048_long": ([3000, 1500, 70], 2048, dict(path="grouped", softmax_nr=0), FULL),
}
SMALL_D = 256
SMALL_RUNS = (("plain", 0.5, True), ("band64", 0.0, True))       # the TRAIN lens of test_gpu_vasnet_lengths.py on the in-loop kernels


def check_regime(cid):
    lens, D, expect, _ = CASES[cid]
    g = regime(lens, D)
    for k, v in expect.items():
        assert g[k] == v, (cid, k, g[k], v, g)
    return g


# ------------------------------------------------------------------------------------------------ inputs
def make_params(D, seed=11):
    """The weights of test_gpu_vasnet_lengths.make_model (k2 scaled so that the scores stay inside (0.01, 0.99)): {name: fp32 CPU tensor}."""
    m = L.make_model(D, seed, "bf16")
    return {k: v.detach().clone() for k, v in m.named_parameters()}, float(np.float32(m.scale)), float(np.float32(m.epsilon))


def make_batch(lens, D):
    """x (R, D) with 4x features at the boundary keys (test_gpu_vasnet_lengths.make_inputs) and seeded normal loss weights, fp32 CPU."""
    x = L.make_inputs(lens, D, seed=sum(lens) + D)
    w = torch.from_numpy(np.random.default_rng(W_SEED).standard_normal(sum(lens)).astype(np.float32))
    return x, w


def drop_masks(lens, D, p, seed=SEED):
    return R.vasnet_drop_masks(seed, p, lens, D) if p > 0 else None


def nudge(t, seed):
    """t (fp32) moved by one ulp per element, up or down by a seeded coin."""
    g = torch.Generator().manual_seed(seed)
    up = torch.randint(0, 2, t.shape, generator=g, dtype=torch.bool).to(t.device)
    inf = torch.full_like(t, float("inf"))
    return torch.nextafter(t, torch.where(up, inf, -inf))


# ------------------------------------------------------------------------------------------------ the reference
def port_step(params, x, w, lens, scale, eps, dtype, device, mask="plain", masks=None, fault=None, bf16_products=True, round_leaves=True):
    """One training step of the emulated port in `dtype` on `device`: loss = sum(w * scores), one video at a time.
    params / x / w: fp32 tensors (converted here, so that every member starts from fp32 values); masks: recipes.vasnet_drop_masks(...) or
    None.  fault: a seeded fault for the host test (see FAULTS).  Returns {"logits", "dX", <parameter name>: gradient} in `dtype`."""
    kw = dict(MASKS[mask])
    fault = fault or {}
    if fault.get("no_ignore_self"):
        kw["ignore_self"] = False
    if "aperture_delta" in fault and kw.get("aperture") is not None:
        kw["aperture"] += fault["aperture_delta"]
    p = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in params.items()}
    xd = x.detach().to(device=device, dtype=dtype).requires_grad_(True)
    wd = w.to(device=device, dtype=dtype)
    logits = torch.empty(sum(lens), dtype=dtype, device=device)
    total, r0 = 0, 0
    for v, T in enumerate(lens):
        dm = None
        if masks is not None:
            mv = masks[v]
            if fault.get("alpha_local_rows") == v:                    # the alpha mask drawn for video-local rows (as if the video stood first)
                mv = (R.vasnet_drop_masks(SEED, fault["p"], [T], x.shape[1])[0][0],) + tuple(mv[1:])
            dm = tuple(torch.from_numpy(a).to(device=device, dtype=dtype).unsqueeze(0) for a in mv)
        km = None
        if fault.get("drop_key", (None,))[0] == v:
            km = torch.zeros(1, T, T, dtype=torch.bool, device=device)
            km[:, :, fault["drop_key"][1]] = True
        s, u = torch_port.vasnet_scores(xd[r0:r0 + T].unsqueeze(1), p, scale=scale, eps=eps, drop_masks=dm, return_logits=True,
                                        bf16_products=bf16_products, round_leaves=round_leaves, key_mask=km, **kw)
        total = total + (s[:, 0, 0] * wd[r0:r0 + T]).sum()
        logits[r0:r0 + T] = u[:, 0, 0].detach()
        r0 += T
    total.backward()
    out = {k: v.grad for k, v in p.items()}
    out["dX"], out["logits"] = xd.grad, logits
    return out


def ensemble(params, x, w, lens, scale, eps, device, mask="plain", masks=None):
    """(E64, [members]): the reference and the runs its yardstick is taken from (N_NUDGE nudged float64 runs, one fp32 run)."""
    ref = port_step(params, x, w, lens, scale, eps, torch.float64, device, mask, masks)
    members = []
    for s in range(N_NUDGE):
        pn = {k: nudge(v, 1000 * (s + 1) + i) for i, (k, v) in enumerate(sorted(params.items()))}
        members.append(port_step(pn, nudge(x, 1000 * (s + 1) + 99), w, lens, scale, eps, torch.float64, device, mask, masks))
    members.append(port_step(params, x, w, lens, scale, eps, torch.float32, device, mask, masks))
    return ref, members


# ------------------------------------------------------------------------------------------------ metric, yardstick, gates
def _row_video(lens, device):
    return torch.repeat_interleave(torch.arange(len(lens), device=device), torch.as_tensor(lens, device=device))


def distances(got, ref, lens):
    """{name: relative L2 distance to ref} over the tensors of `ref` that `got` has: whole tensors, and "dX@v" / "logits@v" per video v.
    Taken over the entries the reference has finite; inf where got is not finite there."""
    out = {}
    dev = ref["logits"].device
    vid = _row_video(lens, dev)
    for k, r in ref.items():
        if k not in got:
            continue
        g = got[k].to(device=dev, dtype=torch.float64).reshape(r.shape)
        r = r.double()
        fin = torch.isfinite(r)
        bad = fin & ~torch.isfinite(g)
        d2 = torch.where(fin & ~bad, (g - r) ** 2, torch.zeros_like(r))
        r2 = torch.where(fin, r ** 2, torch.zeros_like(r))
        rel = lambda n, d: float("inf") if not np.isfinite(n) else float(np.sqrt(n / d)) if d > 0 else float(np.sqrt(n))
        out[k] = float("inf") if bool(bad.any()) else rel(float(d2.sum()), float(r2.sum()))
        if k in ("dX", "logits"):
            rows = lambda t: t.reshape(len(vid), -1).sum(1)
            z = torch.zeros(len(lens), dtype=torch.float64, device=dev)
            n = z.clone().index_add_(0, vid, rows(d2)).cpu().numpy()
            d = z.clone().index_add_(0, vid, rows(r2)).cpu().numpy()
            b = z.clone().index_add_(0, vid, rows(bad.double())).cpu().numpy()
            for v in range(len(lens)):
                out[f"{k}@{v}"] = float("inf") if b[v] else rel(n[v], d[v])
    return out


def yardstick(ref, members, lens):
    ds = [distances(m, ref, lens) for m in members]
    return {k: max(d[k] for d in ds) for k in ds[0]}


def gate_of(yard):
    return max(MULT * yard, FLOOR)


def judge(tag, got, ref, yard, lens, info=None, quiet=False):
    """Compare `got` with the reference: returns (record, [(name, err, yardstick, gate)] of what is over its gate).  The record (every
    error, yardstick, gate and err / yardstick) is appended to REPORT."""
    err = distances(got, ref, lens)
    rows, bad = {}, []
    for k, e in err.items():
        y = yard[k]
        gt = gate_of(y)
        rows[k] = dict(err=e, yardstick=y, gate=gt, ratio=e / max(y, FLOOR / MULT))
        if not e <= gt:
            bad.append((k, e, y, gt))
    worst = max(rows, key=lambda k: rows[k]["ratio"])
    rec = dict(tag=tag, **(info or {}), worst=worst, worst_ratio=rows[worst]["ratio"], tensors=rows)
    REPORT.append(rec)
    if not quiet:
        print(f"\nBF16-F64 {tag}: worst err / yardstick {rows[worst]['ratio']:.3g} on {worst}; over the gate: {len(bad)}")
        for k in list(MATS) + ["dX", "logits"]:
            if k in rows:
                print(f"   {k:34s} err {rows[k]['err']:.3e}  yardstick {rows[k]['yardstick']:.3e}  gate {rows[k]['gate']:.3e}  ratio {rows[k]['ratio']:.3g}")
    return rec, bad


def nan_pattern_equal(got, ref):
    """NaN exactly where the reference has NaN, for every tensor of ref that got has."""
    return all(torch.equal(torch.isnan(got[k]).reshape(-1).cpu(), torch.isnan(r).reshape(-1).cpu()) for k, r in ref.items() if k in got)
