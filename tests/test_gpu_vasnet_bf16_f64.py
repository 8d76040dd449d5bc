"""GPU: VASNet's mixed-precision training step (precision="bf16": forward, every parameter gradient, dX) on EVERY length path of
csrc/vasnet.hip against the float64 emulation of the same arithmetic (tests/vasnet_bf16_common.py, whose docstring lists the rounding
points the reference assumes and where each was read in the source).

Paths, restated per case by vasnet_bf16_common.regime and asserted:
  fused     use_b16 and t_max <= 320: attention on the strips of attn_b16.hip                                            fused_320
  grouped   use_b16 and t_max > 320: attn_grouped() and the non-fused branch of backward_dense() on the per-video bf16-source GEMMs
            (Q.K^T from qkv16, alpha.V / dV from p16 with K = T and ld16 = T rounded up to 64, dQ / dK from bf16(dLogits) written over
            p16), vasnet_softmax_kernel<8 | 16 | 0> writing p16, vasnet_softmax_bwd_kernel<0> writing s16          every other case
  inloop    use_b16 false (fewer than 512 tiles of 128 x 128): the converting kernels of gemm_split.hip               the small batches
Wide-tile BM of the row-wise problems (gemm_b16_wide_bm): 256 for (R, 3D) and 192 for (R, D) in every case of the table (D = 1024 with
R = 8092 ... 8198, and D = 2048 with R = 4570) -- both heights run in every case; the JSON report has them per run.

Each run: logits (recovered from the scores) and every gradient within MULT x the reference-only yardstick, per tensor and, for dX and
the logits, per video; NaN exactly where the reference has NaN; a second run with every fresh workspace, output and shadow handed out
as 0xFF bytes (NaN as fp32 and bf16) bit-identical -- p16 / s16 pad columns and K-tail reads past a video would show there.  Runs per
case: dropout 0.5 with dX under masks plain / ignore_self / aperture 64, dropout 0, and want_dx=False (the (b16 && !dx) branch that never
writes fp32 dY0).  One test re-runs two grouped cases in a child process with SUMK_BF16_SRC=0: other bits, so the cases above did run
the bf16-source kernels.

Measured on MI355X (profiles/vasnet_bf16_f64_report.json, written with SUMK_BF16_LENGTHS_REPORT set): all 63 runs pass with MULT = 4.
Whole tensors: err / yardstick at most 0.92 (k2.bias of stream_1025 without dropout; yardsticks 3e-5 ... 5e-2).  Per video: at most
1.93, on dX of the 33-frame video of grouped_1024 (err 2.7e-2, yardstick 1.4e-2), then 1.003 on the logits of the 2-frame video of
fused_320 under ignore_self (err 7.1e-5); every other slice is below 0.91.  The in-loop small batches stay below 0.70.  The smallest seeded-fault ratio of tests/test_vasnet_bf16_host.py is 44.6 (aperture off by one),
which caps MULT at 11; it stays at 4."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vasnet_bf16_common as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = B.L


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    prev = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32, torch.get_float32_matmul_precision())
    torch.backends.cuda.matmul.allow_tf32 = False           # the fp32 member of the ensemble: IEEE fp32 products
    torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    yield torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = prev[:2]
    torch.set_float32_matmul_precision(prev[2])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    B.dump_report()


# ------------------------------------------------------------------------------------------------ the HIP step
class _Poison:
    """Every workspace and every torch.empty / empty_like on the GPU comes back filled with 0xFF while this is active."""

    def __enter__(self):
        from summarizer_amd import kernels
        self.saved = (torch.empty, torch.empty_like, kernels.workspace)
        empty, empty_like, ws = self.saved

        def fill(t):
            if isinstance(t, torch.Tensor) and t.is_cuda and t.numel() and t.is_contiguous():
                t.reshape(-1).view(torch.uint8).fill_(255)
            return t
        torch.empty, torch.empty_like = (lambda *a, **k: fill(empty(*a, **k))), (lambda *a, **k: fill(empty_like(*a, **k)))
        kernels.workspace = lambda *a, **k: fill(ws(*a, **k))
        for buf in kernels._ws_cache.values():
            buf.fill_(255)
        return self

    def __exit__(self, *exc):
        from summarizer_amd import kernels
        torch.empty, torch.empty_like, kernels.workspace = self.saved


def hip_step(m, x, w, lens, p, want_dx):
    """One training step through the library: {"scores", "dX" (want_dx), <parameter name>: gradient}, fp32."""
    from summarizer_amd import kernels
    from summarizer_amd.autograd import VasnetFunction
    names = [k for _, k in kernels.VASNET_FIELDS]
    params = dict(m.named_parameters())
    for q in params.values():
        q.grad = None
    kernels.drop_shadows(x)
    xp = x.detach().clone().requires_grad_(True) if want_dx else x
    sb = kernels.SeqBatch.get(lens, x.device)
    opts = dict(scale=float(m.scale), eps=float(m.epsilon), ignore_self=bool(m.ignore_self), aperture=m.aperture, dropout_p=float(p), seed=B.SEED,
                precision="bf16")
    s = VasnetFunction.apply(xp, sb, opts, None, None, names, *[params[n] for n in names])
    (s * w).sum().backward()
    out = {k: params[k].grad.detach().clone() for k in names}
    out["scores"] = s.detach().clone()
    if want_dx:
        out["dX"] = xp.grad.detach().clone()
    return out


_BATCH = {}


def batch(dev, lens, D, p):
    key = (tuple(lens), D)
    if _BATCH.get("key") != key:
        _BATCH.clear()
        x, w = B.make_batch(lens, D)
        _BATCH.update(key=key, x=x, w=w, xd=x.to(dev), wd=w.to(dev), params=B.make_params(D), masks={})
    if p not in _BATCH["masks"]:
        _BATCH["masks"][p] = B.drop_masks(lens, D, p)
    return _BATCH


_REF = {}


def reference(dev, lens, D, mask, p):
    """(E64, yardstick) of a (batch, mask, dropout): computed once, shared by the runs that need it."""
    key = (tuple(lens), D, mask, p)
    if key not in _REF:
        b = batch(dev, lens, D, p)
        params, scale, eps = b["params"]
        ref, members = B.ensemble(params, b["x"], b["w"], lens, scale, eps, dev, mask, b["masks"][p])
        _REF[key] = (ref, B.yardstick(ref, members, lens))
    return _REF[key]


def hip_case(dev, lens, D, mask, p, want_dx, poisoned=False):
    b = batch(dev, lens, D, p)
    m = L.make_model(D, 11, "bf16", **B.MASKS[mask]).to(dev)
    if poisoned:
        with _Poison():
            return hip_step(m, b["xd"], b["wd"], lens, p, want_dx)
    return hip_step(m, b["xd"], b["wd"], lens, p, want_dx)


def _logit(s):
    s = s.double()
    return torch.log(s) - torch.log1p(-s)


def check(dev, tag, lens, D, mask, p, want_dx, g):
    ref, yard = reference(dev, lens, D, mask, p)
    s64 = torch.sigmoid(ref["logits"])
    assert float(s64.min()) > 0.01 and float(s64.max()) < 0.99, (float(s64.min()), float(s64.max()))
    a = hip_case(dev, lens, D, mask, p, want_dx)
    b = hip_case(dev, lens, D, mask, p, want_dx, poisoned=True)
    assert ("dX" in a) == want_dx
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (tag, k, "changed after workspaces and outputs were poisoned")
    got = dict(a, logits=_logit(a.pop("scores")))
    assert B.nan_pattern_equal(got, ref), (tag, "NaN where the reference is finite or the other way round")
    info = dict(mask=mask, dropout=p, want_dx=want_dx, D=D, n_seq=len(lens),
                **{k: g[k] for k in ("path", "R", "t_max", "softmax_nr", "ld16", "bm_qkv", "bm_d")})
    rec, bad = B.judge(tag, got, ref, yard, lens, info)
    assert not bad, (tag, bad[:8])
    return rec


# ------------------------------------------------------------------------------------------------ the matrix
def _run_id(r):
    return f"{r[0]}_p{int(r[1] * 10)}_{'dx' if r[2] else 'nodx'}"


MATRIX = [(cid, run) for cid in B.CASES for run in B.CASES[cid][3]]


@pytest.mark.parametrize("cid,run", MATRIX, ids=[f"{c}-{_run_id(r)}" for c, r in MATRIX])
def test_bf16_step_vs_float64_emulation(dev, cid, run):
    lens, D, _, _ = B.CASES[cid]
    g = B.check_regime(cid)
    assert g["b16"], g
    mask, p, want_dx = run
    check(dev, f"{cid}/{_run_id(run)}", lens, D, mask, p, want_dx, g)


SMALL = [(tid, run) for tid in L.TRAIN for run in B.SMALL_RUNS]


@pytest.mark.parametrize("tid,run", SMALL, ids=[f"{t}-{_run_id(r)}" for t, r in SMALL])
def test_small_batch_bf16_step_vs_float64_emulation(dev, tid, run):
    """use_b16 is false: the in-loop converting kernels (precision bf16 of gemm_split.hip) that a trainer hits on small data.  They round
    at the same points (vasnet_bf16_common docstring): the same reference, the same gates."""
    lens, D = L.TRAIN[tid], B.SMALL_D
    g = B.regime(lens, D)
    assert g["path"] == "inloop" and not g["b16"], g
    mask, p, want_dx = run
    check(dev, f"small_{tid}/{_run_id(run)}", lens, D, mask, p, want_dx, g)


def test_gates_reject_a_step_under_another_mask(dev):
    """The gates are not vacuous on the GPU either: the HIP step of grouped_321 with ignore_self, judged against the plain-mask
    reference, is over its gate on weight gradients and by at least 4 x MULT yardsticks on its worst tensor (measured: 276)."""
    lens, D, _, _ = B.CASES["grouped_321"]
    ref, yard = reference(dev, lens, D, "plain", 0.5)
    a = hip_case(dev, lens, D, "noself", 0.5, True)
    got = dict(a, logits=_logit(a.pop("scores")))
    rec, bad = B.judge("control", got, ref, yard, lens, quiet=True)
    B.REPORT.pop()
    names = {k for k, *_ in bad}
    assert names & set(B.MATS) and rec["worst_ratio"] >= 4 * B.MULT, (sorted(names)[:8], rec["worst_ratio"])


_AB_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, "."); sys.path.insert(0, "tests"); sys.path.insert(0, "tests/golden")
import vasnet_bf16_common as B
import test_gpu_vasnet_bf16_f64 as T
out = {}
for cid in sys.argv[2].split(","):
    lens, D, _, _ = B.CASES[cid]
    got = T.hip_case(torch.device("cuda:0"), lens, D, "plain", 0.5, True)
    out.update({f"{cid}:{k}": v.cpu().numpy() for k, v in got.items()})
np.savez(sys.argv[1], **out)
'''


def test_grouped_cases_run_the_bf16_source_kernels(dev, tmp_path):
    """grouped_321 and stream_1025 with SUMK_BF16_SRC=0 in a child process (the switch is read once per process): the converting kernels
    sum the K slices of the weight gradients in another order, so at least one weight gradient has other bits -- the cases above ran
    the bf16-source kernels."""
    ids = ["grouped_321", "stream_1025"]
    f = tmp_path / "planes.npz"
    r = subprocess.run([sys.executable, "-c", _AB_CHILD, str(f), ",".join(ids)], env=dict(os.environ, SUMK_BF16_SRC="0"), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    other = dict(np.load(f))
    for cid in ids:
        lens, D, _, _ = B.CASES[cid]
        got = hip_case(dev, lens, D, "plain", 0.5, True)
        assert all(np.isfinite(other[f"{cid}:{k}"]).all() for k in got), cid
        assert any(not np.array_equal(got[k].cpu().numpy(), other[f"{cid}:{k}"]) for k in B.MATS), cid
