"""GPU: VASNet's per-video attention (logits, masks, softmax, context) on EVERY sequence-length path of csrc/vasnet.hip against the float64
torch port (oracle/torch_port.vasnet_scores run in float64 on the GPU with plain torch ops).

The kernel sequence is picked from the batch geometry (see `regime` below, which restates each trigger from the source); one case per path:

  F1  fp32 softmax register forms NR = 4 / 8 / 16 and the streaming form     t_max <= 256 / 512 / 1024 / above
  F2  per-video product tiles 64x64 vs 128x128                               mean T = R / n_seq >= 1024
  F3  fp32 small-batch K-slice path (slab softmax)                           R <= SK_MAX_ROWS (1024)
  P0  bf16x6 / bf16x3 without planes (in-loop split kernels)                 fewer than 512 tiles of 128x128 in R x D or R x 3D
  P1  attention strips on planes (attn_pw.hip)                               t_max <= 320, [Q|K|V] planes < 2 GiB
  P2  projections on planes, attention on the in-loop grouped kernels        t_max > 320, t_min < 1536
  P3  as P2 for short videos                                                 t_max <= 320, [Q|K|V] planes >= 2 GiB
  P4  pw_long, qk_direct = 1                                                 t_min >= 1536, R >= Tn, [Q|K] planes < 2 GiB
  P5  pw_long, qk_direct = 0, lone video                                     R < Tn
  P6  pw_long, qk_direct = 0, big batch                                      [Q|K] planes >= 2 GiB

Errors are made visible: k2 is scaled so that the scores stay inside (0.01, 0.99) and the comparison is on logits recovered from the scores;
the frames at key positions where a tile or block edge falls (first / last key of a video, keys 255 / 256, 319 / 320, 511 / 512, 1023 / 1024,
the first key of the last partial 32 / 64 / 256 block and the one before it) have 4x the features of the others, which gives each of them
a large share of the attention of the queries that align with it (about e^8 against a row sum of T e^(1/8)) -- a key that is dropped,
doubled or masked wrongly moves those rows' logits by orders of magnitude more than the gates.

Gates come from arithmetic: the same port run in fp32 on the same inputs is the yardstick (its distance to float64).  fp32 and bf16x6
(fp32-grade products) must stay within 4x the yardstick.  bf16x3 splits each operand into two bf16 planes: hi + lo holds 16 significant bits
(representation error <= 2^-17 relative), and the dropped lo x lo term is <= 2^-18 |a b|, so one product carries ~2^-16 relative error where
an fp32 product rounds to 2^-24: its logit error is bounded by 2^8 x 4 x the fp32 yardstick.  Each case also re-runs after every cached
workspace has been filled with 0xFF (a NaN as fp32 and bf16): bit-identical results, NaN exactly where the reference has NaN (aperture 0 with
ignore_self masks every key)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = (1 << 31) - 65536                         # the plane kernels' 31-bit byte offsets (sumk_internal.h pw_ok, attn_pw.hip attn_pw_ok)
FP32_MULT = 4.0
BF16X3_MULT = 4.0 * 2 ** 8
NP_OF = {"bf16x6": 3, "bf16x3": 2}


# ------------------------------------------------------------------------------------------------ the dispatch, restated from the source
def _pitch(rows):
    return (rows + 63) // 64 * 64                                                  # pw_rows_pitch


def _planes_bytes(rows, K, n):
    return _pitch(rows) * K * n * 2 + 8192                                         # pw_planes_bytes


def _pw_ok(M, N, K, a_rows, b_rows, n):
    return M >= 1 and N % 256 == 0 and K % 32 == 0 and K >= 128 and _planes_bytes(a_rows, K, n) < LIM and _planes_bytes(b_rows, K, n) < LIM


def _tiles128(M, N):
    return -(-M // 128) * -(-N // 128)


def regime(lens, D, precision, training=False):
    """Which kernels csrc/vasnet.hip runs for this batch: geometry() (tile shape, small-batch path), sumk_vasnet_forward (plane path,
    attention on planes, pw_long and its qk_direct form), the softmax form picked from t_max."""
    R, n, t_max, t_min = sum(lens), len(lens), max(lens), min(lens)
    npl = 0 if training else NP_OF.get(precision, 0)
    g = dict(R=R, t_max=t_max, t_min=t_min, softmax_nr=4 if t_max <= 256 else 8 if t_max <= 512 else 16 if t_max <= 1024 else 0,
             tile128=R // n >= 1024, sk=precision == "fp32" and R <= 1024 and D <= 2048)
    small = _tiles128(R, 3 * D) < 512 or _tiles128(R, D) < 512                    # rowwise_small_tile
    pw = bool(npl) and D % 256 == 0 and R >= 256 and not small and _pw_ok(R, 3 * D, D, R, 3 * D, npl)
    pw_attn = pw and t_max <= 320 and _planes_bytes(R, 3 * D, npl) < LIM
    tn, kp = (t_max + 255) // 256 * 256, (t_max + 31) // 32 * 32
    pw_long = pw and not pw_attn and t_min >= 1536 and _pw_ok(t_max, tn, D, tn, tn, npl) and _pw_ok(t_max, D, kp, t_max, D, npl)
    qk_direct = pw_long and R >= tn and _pw_ok(R, 2 * D, D, R, 3 * D, npl) and _planes_bytes(R, 2 * D, npl) < LIM
    g.update(tn=tn, pw=pw, pw_attn=pw_attn, pw_long=pw_long, qk_direct=qk_direct, qkv_planes=_planes_bytes(R, 3 * D, npl) if npl else 0,
             qk_planes=_planes_bytes(R, 2 * D, npl) if npl else 0)
    g["path"] = ("pw_long_direct" if qk_direct else "pw_long_split") if pw_long else "pw_attn" if pw_attn else "pw_inloop" if pw else \
        ("split_inloop" if npl else "sk" if g["sk"] else "fp32")
    return g


# ------------------------------------------------------------------------------------------------ inputs
def _lens_fill(head, lo, hi, min_rows, seed):
    rng = np.random.default_rng(seed)
    lens = list(head)
    while sum(lens) < min_rows:
        lens.append(int(rng.integers(lo, hi + 1)))
    return lens


def boundary_keys(T):
    ks = {0, T - 1}
    ks.update(k for k in (255, 256, 319, 320, 511, 512, 1023, 1024, 1535, 1536) if k < T)
    for b in (32, 64, 256):
        last = (T - 1) // b * b
        ks.update(k for k in (last, last - 1) if 0 <= k < T)
    return sorted(ks)


def make_inputs(lens, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(sum(lens), D, generator=g) * 0.5
    r0 = 0
    for T in lens:
        x[[r0 + k for k in boundary_keys(T)]] *= 4.0
        r0 += T
    return x


def make_model(D, seed, precision, ignore_self=False, aperture=None):
    from summarizer_amd.models.vasnet import VASNet
    torch.manual_seed(seed)
    m = VASNet(input_size=D, ignore_self=ignore_self, attention_aperture=aperture)
    with torch.no_grad():
        m.k2.weight.mul_(0.25)                       # z . w2 ~ N(0, 1/4): scores inside (0.01, 0.99) -- logits recoverable from them
        m.k2.bias.zero_()
    m.precision = precision
    return m


MASKS = {"plain": {}, "noself": dict(ignore_self=True), "band63": dict(aperture=63), "band64": dict(aperture=64),
         "band255": dict(aperture=255), "band0_noself": dict(ignore_self=True, aperture=0)}


# ------------------------------------------------------------------------------------------------ the float64 reference
def port_scores(m, x, lens, dtype, want_grad=False, w=None):
    """Per-video scores (and logits) of the torch port in `dtype` on x's device; videos of one length go through together (B > 1).
    want_grad: the port's parameters require grad and sum(w * scores) is back-propagated; returns the grads too."""
    from oracle import torch_port
    p = {k: v.detach().to(dtype).clone().requires_grad_(want_grad) for k, v in m.named_parameters()}
    xd = x.detach().to(dtype).clone().requires_grad_(want_grad)
    off = np.concatenate([[0], np.cumsum(lens)])
    scores = torch.empty(sum(lens), dtype=dtype, device=x.device)
    logits = torch.empty_like(scores)
    groups = {}
    for i, T in enumerate(lens):
        groups.setdefault(T, []).append(i)
    sc = float(np.float32(m.scale))                  # what the kernels receive
    total = 0
    for T, idx in groups.items():
        rows = torch.cat([torch.arange(off[i], off[i + 1], device=x.device) for i in idx])
        xb = xd[rows].view(len(idx), T, -1).permute(1, 0, 2)
        with torch.set_grad_enabled(want_grad):
            s, u = torch_port.vasnet_scores(xb, p, ignore_self=m.ignore_self, aperture=m.aperture, scale=sc, eps=float(np.float32(m.epsilon)),
                                            return_logits=True)
        s, u = s[:, :, 0].permute(1, 0).reshape(-1), u[:, :, 0].permute(1, 0).reshape(-1)
        if want_grad:
            total = total + (s * w.to(dtype)[rows]).sum()
        scores[rows], logits[rows] = s.detach(), u.detach()
    if not want_grad:
        return scores, logits
    total.backward()
    return scores, logits, {k: v.grad for k, v in p.items()}, xd.grad


def all_masked_rows(lens, ignore_self=False, aperture=None):
    """Rows whose every key is masked (the reference's softmax gives NaN there): ignore_self on a 1-frame video, or aperture 0 with ignore_self."""
    rows = torch.zeros(sum(lens), dtype=torch.bool)
    if ignore_self:
        r0 = 0
        for T in lens:
            if T == 1 or aperture == 0:
                rows[r0:r0 + T] = True
            r0 += T
    return rows


def _logit(s):
    s = s.double()
    return torch.log(s) - torch.log1p(-s)


def _err(s, ref_logits):
    """max |logit(s) - reference logit| over the rows the reference has finite; inf if s is non-finite where the reference is finite."""
    fin = torch.isfinite(ref_logits)
    if not bool(torch.isfinite(s[fin]).all()):
        return float("inf")
    return float((_logit(s[fin]) - ref_logits[fin]).abs().max()) if bool(fin.any()) else 0.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    prev = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32, torch.get_float32_matmul_precision())
    torch.backends.cuda.matmul.allow_tf32 = False           # the fp32 yardstick: IEEE fp32 products, no reduced-precision inputs
    torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    yield torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = prev[:2]
    torch.set_float32_matmul_precision(prev[2])


REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SUMK_LENGTHS_REPORT")      # optional: the per-case numbers as JSON (errors, yardsticks, gates, paths)
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)


def _poison():
    from summarizer_amd import kernels
    for buf in kernels._ws_cache.values():
        buf.fill_(255)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ inference cases
ALL3 = ("fp32", "bf16x6", "bf16x3")
SHORT_MASKS = ("plain", "noself", "band63", "band64", "band255", "band0_noself")
LONG_MASKS = ("plain", "noself", "band255", "band0_noself")
CASES = {
    # id: (lens, D, precisions, masks, expected {regime key: value})
    "F1_nr4_256": ([256, 255, 200, 129, 64, 130], 1024, ALL3, SHORT_MASKS, dict(softmax_nr=4, sk=False, path="fp32")),
    "F1_nr8_257": ([257, 256, 255, 100, 200], 1024, ALL3, SHORT_MASKS, dict(softmax_nr=8, sk=False)),
    "F1_nr8_512": ([512, 511, 33, 100], 1024, ALL3, SHORT_MASKS, dict(softmax_nr=8, sk=False)),
    "F1_nr16_513": ([513, 512, 1, 64], 1024, ALL3, SHORT_MASKS, dict(softmax_nr=16, sk=False)),
    "F1_nr16_1024": ([1024, 1000, 3], 1024, ALL3, SHORT_MASKS, dict(softmax_nr=16, sk=False)),
    "F1_stream_1025": ([1025, 1024, 63], 1024, ALL3, SHORT_MASKS, dict(softmax_nr=0, sk=False)),
    "F2_tile64": ([2000, 47], 1024, ("fp32",), LONG_MASKS, dict(tile128=False, softmax_nr=0)),
    "F2_tile128": ([2000, 48], 1024, ("fp32",), LONG_MASKS, dict(tile128=True, softmax_nr=0)),
    "F3_sk_1024": ([700, 324], 1024, ("fp32",), SHORT_MASKS, dict(sk=True, softmax_nr=16)),
    "F3_nosk_1025": ([700, 325], 1024, ("fp32",), SHORT_MASKS, dict(sk=False, softmax_nr=16)),
    "P0_split_inloop": ([235, 300, 190, 320, 257], 1024, ALL3, SHORT_MASKS, dict(path="split_inloop")),
    "P1_pw_attn_320": (_lens_fill([320, 1, 64, 255, 256, 319], 100, 320, 8065, 1), 1024, ALL3, SHORT_MASKS, dict(path="pw_attn", t_max=320)),
    "P2_t321": (_lens_fill([321, 1, 255, 256, 320], 100, 321, 8065, 2), 1024, ALL3, SHORT_MASKS, dict(path="pw_inloop", t_max=321)),
    "P2_summe": (_lens_fill([650, 100], 100, 650, 8065, 3), 1024, ALL3, SHORT_MASKS, dict(path="pw_inloop", t_max=650)),
    "P2_t1535": ([1535, 1536, 1600], 2048, ALL3, LONG_MASKS, dict(path="pw_inloop", t_min=1535)),
    "P3_pw_inloop_short": (_lens_fill([320, 1], 280, 320, 118000, 4), 1024, ("bf16x6",), ("plain", "band64"), dict(path="pw_inloop", t_max=320)),
    "P4_direct_ragged": ([1600, 2049, 1537], 2048, ALL3, LONG_MASKS, dict(path="pw_long_direct")),
    "P4_direct_lone4096": ([4096], 2048, ALL3, LONG_MASKS, dict(path="pw_long_direct", tn=4096)),
    "P5_split_lone4000": ([4000], 2048, ALL3, LONG_MASKS, dict(path="pw_long_split", tn=4096)),
    "P6_split_big": ([9800, 9757, 9801, 9856, 9700, 9791, 9830, 9744, 9821], 2048, ("bf16x6",), ("plain", "band255"), dict(path="pw_long_split")),
}


def _check_branch(cid, lens, D, prec, expect):
    g = regime(lens, D, prec)
    for k, v in expect.items():
        if k == "path" and (prec == "fp32") != (v in ("fp32", "sk")):
            continue          # (a case named for a split-arithmetic path runs its fp32 pass on the fp32 kernels, and the other way round)
        assert g[k] == v, (cid, prec, k, g[k], v, g)
    # the predicates the long-path cases are named for
    if g["path"] == "pw_long_split" and len(lens) == 1:
        assert g["R"] < g["tn"], g                                            # P5: a lone video's K rows [ceil64(T), Tn) are never written
    if cid.startswith("P6"):
        assert g["qk_planes"] >= LIM and g["R"] >= g["tn"], g                 # P6: qk_direct off because of the 2 GiB limit alone
    if cid.startswith("P3"):
        assert g["qkv_planes"] >= LIM, g                                      # P3: T <= 320 but no attention on planes
    return g


def score_case(cid, dev, masks=None, precs=None):
    """HIP scores of a case: {(mask, precision): (first run, run after poisoning the workspace)}."""
    lens, D, precisions, mnames, _ = CASES[cid]
    x = make_inputs(lens, D, seed=sum(lens) + D).to(dev)
    out = {}
    for mname in (masks or mnames):
        m = make_model(D, 7, "fp32", **MASKS[mname]).to(dev).eval()
        for prec in (precs or precisions):
            m.precision = prec
            m.invalidate_folded()
            with torch.no_grad():
                a = m.score_packed(x, lens).clone()
                _poison()
                b = m.score_packed(x, lens).clone()
            out[(mname, prec)] = (a, b)
    return x, out


@pytest.mark.parametrize("cid", list(CASES))
def test_attention_paths_vs_float64(dev, cid):
    lens, D, precisions, mnames, expect = CASES[cid]
    for prec in precisions:
        _check_branch(cid, lens, D, prec, expect)
    x, hip = score_case(cid, dev)
    for mname in mnames:
        m = make_model(D, 7, "fp32", **MASKS[mname]).to(dev).eval()
        s64, u64 = port_scores(m, x, lens, torch.float64)
        s32, _ = port_scores(m, x, lens, torch.float32)
        fin = torch.isfinite(u64)
        assert torch.equal(fin.cpu(), ~all_masked_rows(lens, **MASKS[mname])), (cid, mname)
        if bool(fin.any()):
            assert float(s64[fin].min()) > 0.01 and float(s64[fin].max()) < 0.99, (float(s64[fin].min()), float(s64[fin].max()))
        yard = _err(s32, u64)
        for prec in precisions:
            a, b = hip[(mname, prec)]
            assert torch.equal(_bits(a), _bits(b)), (cid, mname, prec, "changed after the workspace was poisoned")
            assert torch.equal(torch.isnan(a), ~fin), (cid, mname, prec, "NaN where the reference is finite or the other way round")
            err = _err(a, u64)
            gate = (BF16X3_MULT if prec == "bf16x3" else FP32_MULT) * yard
            REPORT.append(dict(case=cid, mask=mname, precision=prec, path=regime(lens, D, prec)["path"], err=err, yardstick=yard, gate=gate))
            assert err <= gate, (cid, mname, prec, err, yard, gate)


_AB_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import test_gpu_vasnet_lengths as L
out = {}
for cid in sys.argv[2].split(","):
    _, hip = L.score_case(cid, torch.device("cuda:0"), masks=("plain",), precs=("bf16x6",))
    out[cid] = hip[("plain", "bf16x6")][0].cpu().numpy()
np.savez(sys.argv[1], **out)
'''


def test_pw_long_cases_do_not_run_the_in_loop_kernels(dev, tmp_path):
    """The pw_long cases (P4, P5) with `SUMK_PW_LONG=0` in a child process (the switch is read once per process): the in-loop grouped
    kernels give other bits, so the cases above did run pw_long."""
    ids = ["P4_direct_ragged", "P4_direct_lone4096", "P5_split_lone4000"]
    f = tmp_path / "inloop.npz"
    r = subprocess.run([sys.executable, "-c", _AB_CHILD, str(f), ",".join(ids)], env=dict(os.environ, SUMK_PW_LONG="0"), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    other = dict(np.load(f))
    for cid in ids:
        _, hip = score_case(cid, dev, masks=("plain",), precs=("bf16x6",))
        a = hip[("plain", "bf16x6")][0].cpu().numpy()
        assert np.isfinite(a).all() and not np.array_equal(a, other[cid]), cid


# ------------------------------------------------------------------------------------------------ fp32 training step
TRAIN = {
    "nr4_256": [256, 255, 100, 89],
    "nr8_257": [257, 200, 64],
    "nr8_512": [512, 300, 2],
    "nr16_513": [513, 400, 2],
    "nr16_1024": [1024, 700, 33],
    "nr16_1024_lone": [1024],
    "stream_1025": [1025, 600, 3],
    "tile64_2000_47": [2000, 47],
    "tile128_2000_48": [2000, 48],
    "long_ragged": [1600, 700, 1025],
}


@pytest.mark.parametrize("want_dx", [True, False], ids=["dx", "nodx"])
@pytest.mark.parametrize("mname", ["plain", "noself", "band64"])
@pytest.mark.parametrize("tid", list(TRAIN))
def test_fp32_training_step_vs_float64_autograd(dev, tid, mname, want_dx):
    """Forward + backward of the fp32 training path (dropout off: eval()) on the softmax forms NR = 4 / 8 / 16 / streaming, both product
    tile shapes and a long ragged batch: every parameter gradient (and dX) within 4x the fp32 port's distance to float64 autograd (relative
    to the tensor's largest entry, floor 16 fp32 ulps).  The softmax backward takes its register forms from t_max only on the small-batch
    path without dX (csrc/vasnet.hip sumk_vasnet_backward: R <= SK_MAX_ROWS); the large-batch backward always runs the streaming form --
    hence both `want_dx` settings."""
    lens, D = TRAIN[tid], 256
    g = regime(lens, D, "fp32", training=True)
    assert g["softmax_nr"] == {"nr4": 4, "nr8": 8, "nr16": 16}.get(tid.split("_")[0], 0), g
    bwd_nr = g["softmax_nr"] if g["sk"] and not want_dx else 0
    x = make_inputs(lens, D, seed=sum(lens)).to(dev)
    w = torch.from_numpy(np.random.default_rng(len(lens)).standard_normal(sum(lens)).astype(np.float32)).to(dev)
    m = make_model(D, 11, "fp32", **MASKS[mname]).to(dev).eval()
    for p in m.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(want_dx)
    s = m.score_packed(xg, lens)
    (s * w).sum().backward()
    got = {k: v.grad for k, v in m.named_parameters()}
    _, u64, g64, dx64 = port_scores(m, x, lens, torch.float64, want_grad=True, w=w)
    s32, _, g32, dx32 = port_scores(m, x, lens, torch.float32, want_grad=True, w=w)
    if want_dx:
        got["dX"], g64["dX"], g32["dX"] = xg.grad, dx64, dx32
    assert _err(s.detach(), u64) <= FP32_MULT * _err(s32, u64), (tid, mname, _err(s.detach(), u64), _err(s32, u64))
    for k, ref in g64.items():
        scale = float(ref.abs().max())
        yard = float((g32[k].double() - ref).abs().max()) / scale
        err = float((got[k].double() - ref).abs().max()) / scale
        gate = max(FP32_MULT * yard, 16 * 2.0 ** -24)
        REPORT.append(dict(case=f"train_{tid}", mask=mname, precision="fp32", dx=want_dx, softmax_bwd_nr=bwd_nr, tensor=k, err=err, yardstick=yard, gate=gate))
        assert err <= gate, (tid, mname, k, err, yard)
