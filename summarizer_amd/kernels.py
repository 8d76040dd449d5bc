"""Thin Python layer over the C ABI: packed-batch bookkeeping (sequence offsets, workspaces) and
torch.autograd.Function wrappers.  Every arithmetic result comes from libsumk.so; nothing here computes on
the CPU or through torch ops (torch only allocates the buffers and carries the stream)."""
import collections
import ctypes as C
import math
import os
import numpy as np
import torch

from . import _lib
from ._lib import SumkError


def _require_gpu(t, what):
    if not t.is_cuda:
        raise SumkError(f"{what}: expected a GPU tensor, got device={t.device}. summarizer_amd runs only on the "
                        "HIP path (no CPU fallback); move the model and inputs to cuda.")
    if t.dtype != torch.float32:
        raise SumkError(f"{what}: expected float32, got {t.dtype}")


def _ptr(t, what):
    _require_gpu(t, what)
    if not t.is_contiguous():
        raise SumkError(f"{what} must be contiguous")
    return t.data_ptr()


def _check_rows(x, sb, what, col="D"):
    _require_gpu(x, what)
    if not x.is_contiguous() or x.dim() != 2 or x.shape[0] != sb.n_rows:
        raise SumkError(f"{what} must be contiguous (n_rows={sb.n_rows}, {col}), got {tuple(x.shape)}")


def _nonzero(nbytes, name):
    """A workspace-size query's answer; 0 is the library's refusal (its message is in sumk_last_error)."""
    if nbytes == 0:
        _lib.check(-1, name)
    return nbytes


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class SeqBatch:
    """Packed batch geometry: frames of video s are rows [off[s], off[s+1])."""
    _cache = {}

    def __init__(self, lens, device):
        lens = [int(v) for v in lens]
        if len(lens) == 0 or min(lens) <= 0:
            raise SumkError(f"empty video in batch: lens={lens}")
        self.lens = lens
        self.off_host = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens, out=self.off_host[1:])
        self.n_seq = len(lens)
        self.n_rows = int(self.off_host[-1])
        self.device = device
        self.off_dev = torch.from_numpy(self.off_host).to(device)

    @classmethod
    def get(cls, lens, device):
        key = (tuple(int(v) for v in lens), str(device))
        sb = cls._cache.get(key)
        if sb is None:
            if len(cls._cache) > 256:
                cls._cache.clear()
            sb = cls._cache[key] = SeqBatch(lens, device)
        return sb

    def segment_mean(self, v):
        """Per-video mean of a per-frame quantity: v (..., n_rows) -> (..., n_seq).  Two tiny torch ops (index_add + div)
        whatever the number of videos -- the trainers' loss glue, not a compute kernel."""
        if getattr(self, "_seg", None) is None:
            self._seg = torch.repeat_interleave(torch.arange(self.n_seq, device=self.device),
                                                torch.tensor(self.lens, device=self.device))
            self._len_f = torch.tensor(self.lens, dtype=torch.float32, device=self.device)
        out = torch.zeros(v.shape[:-1] + (self.n_seq,), dtype=v.dtype, device=v.device)
        return out.index_add_(v.dim() - 1, self._seg, v) / self._len_f

    @property
    def off_host_p(self):
        return _lib.host_i32(self.off_host)

    @property
    def off_dev_p(self):
        return C.c_void_p(self.off_dev.data_ptr())


_ws_cache = {}


def workspace(nbytes, device, persistent=False):
    """Caller-owned scratch for one call.  Inference reuses one grow-only buffer per (device, stream) -- calls on one stream
    are ordered, calls on different streams (e.g. ingest.StreamingScorer's compute stream next to the default one) must not
    share scratch; a training forward gets its own buffer (it must survive until backward)."""
    if persistent:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _ws_cache[key] = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
    return buf


_ONES = {}


def one(device):
    """A cached float32 scalar 1.0 on `device`: `loss.backward(gradient=kernels.one(dev))` spares autograd's ones_like + fill launch in
    every training step (the root gradient of a scalar loss)."""
    key = str(device)
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones((), dtype=torch.float32, device=device)
    return t


def one_for(loss):
    """The root gradient for `loss.backward(gradient=...)`: one(device) for a float32 GPU scalar, None (autograd's default) otherwise."""
    return one(loss.device) if loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 else None


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _aligned_block(nb, device, out=None):
    """A 256-byte aligned uint8 view of at least nb bytes that carries its backing tensor as `_sumk_keep`.  out: an earlier backing tensor,
    re-used when it is large enough and on `device`."""
    if out is None or out.numel() < nb + 256 or out.device != device:
        out = torch.empty(nb + 256, dtype=torch.uint8, device=device)
    view = out[(out.data_ptr() + 255) // 256 * 256 - out.data_ptr():]
    view._sumk_keep = out
    return view


def _planes_buffer(rows, K, n_planes, device, what, col="K"):
    """An uninitialised KB-plane array (include/sumk.h "KB planes") for a kernel that writes every row up to the pitch, zeros behind `rows`:
    only the slack behind the last sub-array, which row tiles read past, is filled here."""
    nb = _lib.load().sumk_planes_bytes(rows, K, n_planes)
    if nb == 0:
        raise SumkError(f"{what}: rows={rows} {col}={K} planes={n_planes} is not representable ({col} % 16, 2 or 3 planes)")
    out = torch.empty(nb, dtype=torch.uint8, device=device)
    out[nb - 8192:].zero_()
    return out


# ------------------------------------------------------------------------------------------------ VASNet
VASNET_FIELDS = [("Wk", "K.weight"), ("Wq", "Q.weight"), ("Wv", "V.weight"), ("Wo", "attention_head_projection.weight"),
                 ("W1", "k1.weight"), ("b1", "k1.bias"), ("w2", "k2.weight"), ("b2", "k2.bias"),
                 ("ln_w", "layer_norm.weight"), ("ln_b", "layer_norm.bias")]


PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16x6": 2, "bf16": 3}      # SUMK_PRECISION_* of include/sumk.h


def precision_code(p):
    """"fp32" (default: exact fp32 MFMA), "bf16x6" (fp32-grade, 6 bf16 MFMAs per product), "bf16x3" (hi+lo bf16 split, 3 MFMAs)
    or "bf16" (plain bf16 operands, 1 MFMA, fp32 accumulate: mixed-precision TRAINING arithmetic, ~2^-9 per product)."""
    if p is None:
        return 0
    if p not in PRECISIONS:
        raise SumkError(f"unknown precision {p!r}; expected one of {sorted(PRECISIONS)}")
    return PRECISIONS[p]


def vasnet_tables(sb, D, training, precision_id):
    """The batch's problem tables (sumk_vasnet_opts.tables), built once per (SeqBatch, D, training, arithmetic) and kept with the
    SeqBatch: they depend on the batch geometry only, so no table-setup kernel runs per call.  One buffer per CURRENT stream (the tables
    hold the tickets of the in-launch split-K launches: calls on different streams must not share them)."""
    key = (int(D), int(bool(training)), int(precision_id), torch.cuda.current_stream(sb.device).cuda_stream)
    tabs = getattr(sb, "_vasnet_tables", None)
    if tabs is None:
        tabs = sb._vasnet_tables = {}
    t = tabs.get(key)
    if t is None:
        lib = _lib.load()
        nb = _nonzero(lib.sumk_vasnet_tables_bytes(int(D), sb.n_seq, sb.off_host_p), "sumk_vasnet_tables_bytes")
        t = _aligned_block(nb, sb.device)
        _lib.check(lib.sumk_vasnet_build_tables(int(D), sb.n_seq, sb.off_host_p, sb.off_dev_p, key[1], key[2], _p(t), nb, _stream()),
                   "sumk_vasnet_build_tables")
        tabs[key] = t
    return t.data_ptr()


def _vasnet_structs(params, opts):
    w = _lib.VasnetWeights()
    for f, k in VASNET_FIELDS:
        setattr(w, f, _ptr(params[k], f"VASNet weight {k}"))
    o = _lib.VasnetOpts(float(opts["scale"]), float(opts["eps"]), int(bool(opts.get("ignore_self", False))),
                        -1 if opts.get("aperture") is None else int(opts["aperture"]),
                        float(opts.get("dropout_p", 0.0)), int(opts.get("seed", 0)), precision_code(opts.get("precision")),
                        opts["seed_dev"].data_ptr() if opts.get("seed_dev") is not None else None, opts.get("tables"),
                        opts["x16"].data_ptr() if opts.get("x16") is not None else None,
                        opts["xplanes"].data_ptr() if opts.get("xplanes") is not None else None,
                        opts["wplanes"].data_ptr() if opts.get("wplanes") is not None else None)
    return w, o


def vasnet_wplanes(params, D, n_planes, wvo=None, out=None):
    """The weight-plane block of the plane path (sumk_vasnet_opts.wplanes) for the current weights: planes of [Wq; Wk; Wv] (or Wvo),
    Wo, W1 diag(ln_w) and the fused tail's column vectors.  Returns a 256-byte aligned uint8 tensor, or None when D is not eligible."""
    lib = _lib.load()
    nb = lib.sumk_vasnet_wplanes_bytes(int(D), int(n_planes))
    if nb == 0:
        return None
    w = _lib.VasnetWeights()
    for f, k in VASNET_FIELDS:
        setattr(w, f, params[k].data_ptr())
    view = _aligned_block(nb, params[VASNET_FIELDS[0][1]].device, out)
    _lib.check(lib.sumk_vasnet_wplanes_build(int(D), C.byref(w), _p(wvo), int(n_planes), _p(view), nb, _stream()), "sumk_vasnet_wplanes_build")
    return view


def tensor_shadow(x, name, build):
    """A value derived from the CONTENTS of tensor x (a bf16 copy, bf16 planes ...), kept ON the tensor object: `build()` runs again when
    x was written to through torch (tensor version counter) and the entry dies with x.  Nothing is keyed by address: a fresh tensor that
    the caching allocator places where an earlier one lived (torch.cat of a new mini-batch every step) has no shadow and gets its own
    (the address-keyed cache handed such a tensor the previous batch's copy).  Writes torch cannot see (a C-ABI kernel
    writing into x) must be followed by `drop_shadows(x)`."""
    d = getattr(x, "_sumk_shadows", None)
    if d is None:
        d = {}
        try:
            x._sumk_shadows = d
        except AttributeError:          # (an object that takes no attributes: no caching)
            return build()
    # a shadow is built by kernels on the CURRENT stream: a call on another stream builds its own rather than read one that may not be finished
    stream = torch.cuda.current_stream(x.device).cuda_stream if x.is_cuda else 0
    hit = d.get(name)
    if hit is not None and hit[0] == x._version and hit[2] == stream:
        return hit[1]
    val = build()
    d[name] = (x._version, val, stream)
    return val


def weights_key(tensors, *extra):
    """What a block derived from weights is keyed by: storage addresses and tensor versions (what torch can see), WEIGHTS_EPOCH (bumped by
    every optimiser step through the C ABI, invisible to torch), `extra` (precision ...) and, last, the current stream: the block is built
    by kernels on it, a call on another stream builds its own."""
    t0 = tensors[0]
    return tuple(t.data_ptr() for t in tensors) + tuple(t._version for t in tensors) + (WEIGHTS_EPOCH[0],) + extra + (
        torch.cuda.current_stream(t0.device).cuda_stream if t0.is_cuda else 0,)


def cached_block(owner, slot, key, build):
    """The block (or list of blocks) `build(out)` makes from owner's weights, kept in owner.<slot> under owner.<slot>_key (a weights_key) and
    rebuilt when the key differs or the block is gone -- stale planes give wrong results, not errors (include/sumk.h).  out: the backing
    tensors of the previous block (`_sumk_keep`) for re-use, but only on the stream that built them: kernels another stream has queued
    may still read the old planes."""
    d = owner.__dict__
    if d.get(slot) is None or d.get(slot + "_key") != key:
        with torch.no_grad():
            val = d[slot] = build(d.get(slot + "_buf") if d.get(slot + "_stream") == key[-1] else None)
        d[slot + "_buf"] = [getattr(b, "_sumk_keep", None) for b in val] if isinstance(val, list) else getattr(val, "_sumk_keep", None)
        d[slot + "_key"], d[slot + "_stream"] = key, key[-1]
    return d[slot]


def drop_shadows(x):
    """Forget every shadow of x (after a write torch's version counter does not see)."""
    if getattr(x, "_sumk_shadows", None):
        x._sumk_shadows.clear()


def pos_shadow(x, key, build):
    """The positional sum (fp32 and / or planes) of a packed INFERENCE batch, kept ON the tensor object x like tensor_shadow's entries, but
    ONE entry per x (a second copy of the batch: a table change replaces it instead of piling up beside it).  `key` carries everything the
    sum depends on beside x's address: x's version, the table's identity / version, WEIGHTS_EPOCH, the stream that built it."""
    hit = getattr(x, "_sumk_pos", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    val = build()
    try:
        x._sumk_pos = (key, val)
    except AttributeError:          # (an object that takes no attributes: no caching)
        pass
    return val


def vasnet_x16(x, sb=None):
    """bf16(x) for the mixed-precision training step (sumk_vasnet_opts.x16): kept with the tensor OBJECT while its contents are unchanged
    (tensor_shadow) -- features packed once are constant over the epochs of a run; a loop that packs a fresh batch every step converts per
    call as before."""
    lib = _lib.load()

    def build():
        x16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        _lib.check(lib.sumk_cast_f32_bf16(_p(x), _p(x16), x.numel(), _stream()), "sumk_cast_f32_bf16")
        return x16
    return tensor_shadow(x, "x16", build)


# ------------------------------------------------------------------------------------------------ KB planes (csrc/gemm_pw.hip)
PLANES_OF = {"bf16x6": 3, "bf16x3": 2}      # planes per operand of the split-bf16 arithmetics


def split_planes(x, n_planes):
    """fp32 (rows, K) row-major GPU tensor -> its KB-plane array (uint8 tensor; layout: include/sumk.h "KB planes")."""
    lib = _lib.load()
    _require_gpu(x, "split_planes")
    if x.dim() != 2 or x.stride(1) != 1 or x.stride(0) % 4 != 0:
        raise SumkError("split_planes: a 2-D row-major tensor with a leading dimension that is a multiple of 4")
    rows, K = x.shape
    out = _planes_buffer(rows, K, n_planes, x.device, "split_planes")
    _lib.check(lib.sumk_split_planes(_p(x), rows, K, x.stride(0), n_planes, _p(out), _stream()), "sumk_split_planes")
    return out


def gemm_planes(a_planes, a_rows, b_planes, b_rows, M, N, K, n_planes, variant=0, out=None):
    """C (M, N) fp32 = A . B^T from two KB-plane arrays (tests / bench probe of the plane-aware wide GEMM)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a_planes.device)
    _lib.check(lib.sumk_gemm_planes(_p(a_planes), a_rows, _p(b_planes), b_rows, _p(out), M, N, K, n_planes, variant, _stream()), "sumk_gemm_planes")
    return out


def pos_add_packed(x, sb, table, want_f32=True, want_bf16=False, n_planes=0):
    """Positional embedding of a packed batch, out of place (csrc/posembed.hip): row off[v] + t gets table[t].  Returns
    (fp32 sum or None, its bf16 rounding or None, its KB planes or None) -- whichever of the three were asked for, from ONE launch;
    x is never written."""
    lib = _lib.load()
    _require_gpu(x, "pos_add_packed input"); _require_gpu(table, "pos_add_packed table")
    _check_rows(x, sb, "pos_add_packed: input")
    D = x.shape[1]
    if table.dim() != 2 or table.shape[1] != D or not table.is_contiguous() or table.device != x.device:
        raise SumkError(f"pos_add_packed: table must be contiguous (max_length, {D}) on {x.device}, got {tuple(table.shape)} on {table.device}")
    y32 = torch.empty_like(x) if want_f32 else None
    y16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    planes = _planes_buffer(sb.n_rows, D, n_planes, x.device, "pos_add_packed", col="D") if n_planes else None
    _lib.check(lib.sumk_pos_add_packed(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, _p(table), table.shape[0], _p(y32), _p(y16), _p(planes),
                                       int(n_planes), _stream()), "sumk_pos_add_packed")
    return y32, y16, planes


def pos_table_grad(dx, sb, dtable):
    """dtable[t] += sum over the batch's videos longer than t of dx[off[v] + t], videos in ascending order (deterministic; csrc/posembed.hip)."""
    _require_gpu(dx, "pos_table_grad dx"); _require_gpu(dtable, "pos_table_grad dtable")
    if not dx.is_contiguous():
        dx = dx.contiguous()
    if dx.dim() != 2 or dx.shape[0] != sb.n_rows or dtable.dim() != 2 or dtable.shape[1] != dx.shape[1] or not dtable.is_contiguous():
        raise SumkError(f"pos_table_grad: dx {tuple(dx.shape)} / dtable {tuple(dtable.shape)} do not fit {sb.n_rows} rows (contiguous, same D)")
    _lib.check(_lib.load().sumk_pos_table_grad(_p(dx), dx.shape[1], sb.n_seq, sb.off_host_p, sb.off_dev_p, _p(dtable), dtable.shape[0], _stream()),
               "sumk_pos_table_grad")


def fold_vo(w_o, w_v, out=None):
    """Wvo = Wo . Wv (D, D) for the folded inference path (sumk_vasnet_forward_folded); one fp32 MFMA GEMM."""
    lib = _lib.load()
    _require_gpu(w_o, "fold_vo"); _require_gpu(w_v, "fold_vo")
    D = w_o.shape[0]
    if out is None:
        out = torch.empty(D, D, dtype=torch.float32, device=w_o.device)
    _lib.check(lib.sumk_gemm_nn(_p(w_o.contiguous()), _p(w_v.contiguous()), _p(out), D, D, D, _stream()), "sumk_gemm_nn (fold_vo)")
    return out


def vasnet_forward_packed(x, sb, params, opts, pos_table=None, pos_rows=None, training=False, wvo=None):
    """x: (n_rows, D) packed, contiguous, on GPU.  Returns (scores (n_rows,), workspace or None).
    wvo: folded Wo.Wv (inference only) -> the output projection is absorbed into the packed projection (fold_vo)."""
    lib = _lib.load()
    _check_rows(x, sb, "vasnet input")
    D = x.shape[1]
    # Entries this function derives (tables of the batch geometry, the bf16 / plane shadows of x) are written back into `opts` so that the
    # backward pass of the same step finds them; they are tied to THIS (x, batch): a caller that re-uses the dict for another batch gets
    # them rebuilt instead of silently scoring with the first batch's planes (sumk.h: stale planes give wrong results, not errors).
    dkey = (x.data_ptr(), x._version, tuple(x.shape), id(sb))
    if opts.get("_derived_for") != dkey:
        for k in opts.pop("_derived", ()):
            opts.pop(k, None)
        opts["_derived_for"], opts["_derived"] = dkey, []
    if "tables" not in opts and not torch.cuda.is_current_stream_capturing():      # (built outside a capture; a captured call reuses what exists)
        opts["tables"] = vasnet_tables(sb, D, training, precision_code(opts.get("precision"))); opts["_derived"].append("tables")
    elif "tables" not in opts:
        # inside a capture nothing may be allocated or built for the (private) capture stream: the step reuses the tables an eager call
        # of the same geometry built before (a replay runs where the eager calls ran); none yet -> the setup kernel is captured instead
        want = (int(D), int(bool(training)), precision_code(opts.get("precision")))
        hit = [v for k, v in getattr(sb, "_vasnet_tables", {}).items() if k[:3] == want]
        opts["tables"] = hit[-1].data_ptr() if hit else None; opts["_derived"].append("tables")
    if (training and "x16" not in opts and precision_code(opts.get("precision")) == precision_code("bf16") and pos_table is None
            and x.numel() % 4 == 0 and not x.requires_grad and not torch.cuda.is_current_stream_capturing()):
        opts["x16"] = vasnet_x16(x, sb); opts["_derived"].append("x16")        # (an input that asks for dX is an activation, not a dataset: cast per call)
    n_planes = PLANES_OF.get(opts.get("precision"))
    if (n_planes and not training and "xplanes" not in opts and opts.get("wplanes") is not None and pos_table is None
            and D % 256 == 0 and sb.n_rows >= 256 and not torch.cuda.is_current_stream_capturing()):
        # plane path (csrc/gemm_pw.hip): the operand planes of x are kept with the tensor object (constant per dataset)
        opts["xplanes"] = tensor_shadow(x, f"planes{n_planes}", lambda: split_planes(x, n_planes)); opts["_derived"].append("xplanes")
    w, o = _vasnet_structs(params, opts)
    nbytes = _nonzero(lib.sumk_vasnet_workspace_bytes_for(D, sb.n_seq, sb.off_host_p, int(training), int(o.precision)), "sumk_vasnet_workspace_bytes_for")
    ws = workspace(nbytes, x.device, persistent=training)
    scores = torch.empty(sb.n_rows, dtype=torch.float32, device=x.device)
    if wvo is not None:
        if training:
            raise SumkError("vasnet: the folded projection is inference-only")
        rc = lib.sumk_vasnet_forward_folded(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(w), _p(wvo), C.byref(o),
                                            _p(pos_table), _p(pos_rows), _p(scores), _p(ws), ws.numel(), _stream())
    else:
        rc = lib.sumk_vasnet_forward(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(w), C.byref(o),
                                     _p(pos_table), _p(pos_rows), _p(scores), _p(ws), ws.numel(), int(training), _stream())
    _lib.check(rc, "sumk_vasnet_forward")
    return scores, (ws if training else None)


# ------------------------------------------------------------------------------------------------ local attention on the band
ATTN_BAND_MAX_STEPS = 1048576      # per video: sumk_attn_band / sumk_vasnet_forward_band (include/sumk.h)


def _band_aperture(aperture, what):
    if not isinstance(aperture, (int, np.integer)) or isinstance(aperture, bool) or aperture < 0:
        raise SumkError(f"{what}: the band needs an int aperture >= 0, got {aperture!r}")
    return int(min(aperture, 2 ** 31 - 1))


def attn_band_workspace_bytes(D, sb, aperture):
    """Bytes sumk_attn_band needs for this batch: pure host arithmetic, 0 for arguments it would refuse."""
    return _lib.load().sumk_attn_band_workspace_bytes(int(D), sb.n_seq, sb.off_host_p, int(aperture))


def vasnet_band_workspace_bytes(D, sb, aperture):
    """Bytes sumk_vasnet_forward_band needs for this batch: pure host arithmetic, 0 for arguments it would refuse."""
    return _lib.load().sumk_vasnet_band_workspace_bytes(int(D), sb.n_seq, sb.off_host_p, int(aperture))


def attn_band(q, k, v, sb, aperture, scale, ignore_self=False, want_alpha=False):
    """Per video of the packed batch, ctx = softmax(mask(q k^T * scale)) v over the keys [i - aperture, i + aperture] of every query row i
    (sumk_attn_band, include/sumk.h): O(T aperture) workspace and work.  q, k, v: (n_rows, D) views with unit column stride (e.g. column
    blocks of one (n_rows, 3 D) projection).  Returns (ctx (n_rows, D), alpha (n_rows, 2 aperture + 1) or None); alpha[i, c] is the weight
    of key i - aperture + c, zero outside the video.  Only enqueues work on the current stream."""
    lib = _lib.load()
    w = _band_aperture(aperture, "attn_band")
    D = q.shape[1] if q.dim() == 2 else -1
    for name, t in (("q", q), ("k", k), ("v", v)):
        _require_gpu(t, f"attn_band {name}")
        if t.dim() != 2 or t.shape != (sb.n_rows, D) or t.stride(1) != 1:
            raise SumkError(f"attn_band: {name} must be ({sb.n_rows}, D) with unit column stride, got {tuple(t.shape)} strides {t.stride()}")
    nb = _nonzero(lib.sumk_attn_band_workspace_bytes(D, sb.n_seq, sb.off_host_p, w), "sumk_attn_band_workspace_bytes")
    ws = workspace(nb, q.device)
    ctx = torch.empty(sb.n_rows, D, dtype=torch.float32, device=q.device)
    alpha = torch.empty(sb.n_rows, 2 * w + 1, dtype=torch.float32, device=q.device) if want_alpha else None
    _lib.check(lib.sumk_attn_band(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), D, sb.n_seq, sb.off_host_p, sb.off_dev_p,
                                  float(scale), int(bool(ignore_self)), w, _p(ctx), D, _p(alpha), _p(ws), ws.numel(), _stream()), "sumk_attn_band")
    return ctx, alpha


def vasnet_forward_band(x, sb, params, opts):
    """VASNet inference with the attention on the band (sumk_vasnet_forward_band): x (n_rows, D) packed -> scores (n_rows,).  opts as for
    vasnet_forward_packed; needs an int aperture >= 0, exact fp32 and no dropout.  x is not modified.  Only enqueues work."""
    lib = _lib.load()
    _check_rows(x, sb, "vasnet input")
    D = x.shape[1]
    w = _band_aperture(opts.get("aperture"), "vasnet_forward_band")
    wts, o = _vasnet_structs(params, dict({k: v for k, v in opts.items() if k not in ("tables", "x16", "xplanes", "wplanes")}, aperture=w))
    nb = _nonzero(lib.sumk_vasnet_band_workspace_bytes(D, sb.n_seq, sb.off_host_p, w), "sumk_vasnet_band_workspace_bytes")
    ws = workspace(nb, x.device)
    scores = torch.empty(sb.n_rows, dtype=torch.float32, device=x.device)
    _lib.check(lib.sumk_vasnet_forward_band(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(wts), C.byref(o), _p(scores), _p(ws),
                                            ws.numel(), _stream()), "sumk_vasnet_forward_band")
    return scores


def attn_band_train_workspace_bytes(D, sb, aperture):
    """Bytes a training call of the band attention needs (three rectangle buffers): pure host arithmetic, 0 for arguments it would refuse."""
    return _lib.load().sumk_attn_band_train_workspace_bytes(int(D), sb.n_seq, sb.off_host_p, int(aperture))


def vasnet_band_train_workspace_bytes(D, sb, aperture):
    """Bytes sumk_vasnet_forward_band_train / _backward_band need for this batch: pure host arithmetic, 0 for arguments they would refuse."""
    return _lib.load().sumk_vasnet_band_train_workspace_bytes(int(D), sb.n_seq, sb.off_host_p, int(aperture))


def _band_rows(what, sb, D, **tensors):
    for name, t in tensors.items():
        _require_gpu(t, f"{what} {name}")
        if t.dim() != 2 or t.shape != (sb.n_rows, D) or t.stride(1) != 1:
            raise SumkError(f"{what}: {name} must be ({sb.n_rows}, D) with unit column stride, got {tuple(t.shape)} strides {t.stride()}")


def _seed_dev_p(seed_dev):
    return C.c_void_p(seed_dev.data_ptr()) if seed_dev is not None else C.c_void_p(0)


def attn_band_train(q, k, v, sb, aperture, scale, ignore_self=False, dropout_p=0.0, seed=0, seed_dev=None, ctx=None, ws=None):
    """`attn_band` in training mode (sumk_attn_band_forward_train): dropout of the weights at site 0 with the dense path's index, and the
    workspace keeps alpha / dropout(alpha) for `attn_band_backward`.  Returns (ctx, ws).  ctx / ws: buffers to write into (a caller that
    captures the call, or checks what it leaves untouched).  Only enqueues work on the current stream."""
    lib = _lib.load()
    w = _band_aperture(aperture, "attn_band_train")
    D = q.shape[1] if q.dim() == 2 else -1
    _band_rows("attn_band_train", sb, D, q=q, k=k, v=v)
    if ws is None:
        nb = _nonzero(lib.sumk_attn_band_train_workspace_bytes(D, sb.n_seq, sb.off_host_p, w), "sumk_attn_band_train_workspace_bytes")
        ws = workspace(nb, q.device, persistent=True)
    if ctx is None:
        ctx = torch.empty(sb.n_rows, D, dtype=torch.float32, device=q.device)
    _lib.check(lib.sumk_attn_band_forward_train(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), D, sb.n_seq, sb.off_host_p,
                                                sb.off_dev_p, float(scale), int(bool(ignore_self)), w, float(dropout_p), int(seed),
                                                _seed_dev_p(seed_dev), _p(ctx), ctx.stride(0), _p(ws), ws.numel(), _stream()),
               "sumk_attn_band_forward_train")
    return ctx, ws


def attn_band_backward(q, k, v, dctx, sb, aperture, scale, ws, ignore_self=False, dropout_p=0.0, seed=0, seed_dev=None, out=None):
    """Gradients of `attn_band_train` (sumk_attn_band_backward): (dq, dk, dv), each (n_rows, D), from dctx and the workspace the forward
    left; the options must be the forward's.  out: three buffers to write into.  Only enqueues work on the current stream."""
    lib = _lib.load()
    w = _band_aperture(aperture, "attn_band_backward")
    D = q.shape[1] if q.dim() == 2 else -1
    _band_rows("attn_band_backward", sb, D, q=q, k=k, v=v, dctx=dctx)
    if not ws.is_cuda:
        raise SumkError("attn_band_backward: the workspace must be the GPU buffer attn_band_train returned")
    dq, dk, dv = out if out is not None else (torch.empty(sb.n_rows, D, dtype=torch.float32, device=q.device) for _ in range(3))
    _band_rows("attn_band_backward", sb, D, dq=dq, dk=dk, dv=dv)
    _lib.check(lib.sumk_attn_band_backward(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(dctx), dctx.stride(0), D, sb.n_seq,
                                           sb.off_host_p, sb.off_dev_p, float(scale), int(bool(ignore_self)), w, float(dropout_p), int(seed),
                                           _seed_dev_p(seed_dev), _p(dq), dq.stride(0), _p(dk), dk.stride(0), _p(dv), dv.stride(0), _p(ws),
                                           ws.numel(), _stream()), "sumk_attn_band_backward")
    return dq, dk, dv


def _band_structs(params, opts, what):
    w = _band_aperture(opts.get("aperture"), what)
    return _vasnet_structs(params, dict({k: v for k, v in opts.items() if k not in ("tables", "x16", "xplanes", "wplanes")}, aperture=w)) + (w,)


def vasnet_forward_band_train(x, sb, params, opts, ws=None):
    """VASNet's training-mode forward with the attention on the band (sumk_vasnet_forward_band_train): x (n_rows, D) packed ->
    (scores (n_rows,), workspace for `vasnet_backward_band`).  opts as for vasnet_forward_packed with an int aperture >= 0 and exact fp32;
    x is not modified.  Only enqueues work."""
    lib = _lib.load()
    _check_rows(x, sb, "vasnet input")
    D = x.shape[1]
    wts, o, w = _band_structs(params, opts, "vasnet_forward_band_train")
    if ws is None:
        nb = _nonzero(lib.sumk_vasnet_band_train_workspace_bytes(D, sb.n_seq, sb.off_host_p, w), "sumk_vasnet_band_train_workspace_bytes")
        ws = workspace(nb, x.device, persistent=True)
    scores = torch.empty(sb.n_rows, dtype=torch.float32, device=x.device)
    _lib.check(lib.sumk_vasnet_forward_band_train(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(wts), C.byref(o), _p(scores), _p(ws),
                                                  ws.numel(), _stream()), "sumk_vasnet_forward_band_train")
    return scores, ws


def vasnet_backward_band(x, sb, params, opts, dscores, ws, grads, want_dx=False):
    """`vasnet_backward_packed` for a step whose forward was `vasnet_forward_band_train`: ACCUMULATES the weight gradients into `grads`,
    returns dx (or None)."""
    lib = _lib.load()
    _check_rows(x, sb, "vasnet input")
    D = x.shape[1]
    wts, o, _ = _band_structs(params, opts, "vasnet_backward_band")
    g = _lib.VasnetGrads()
    for f, k in VASNET_FIELDS:
        t = grads[k]
        _require_gpu(t, f"VASNet grad {k}")
        setattr(g, f, t.data_ptr())
    dx = torch.empty_like(x) if want_dx else None
    if not dscores.is_contiguous():
        dscores = dscores.contiguous()
    ev = opts.get("tail_grads_ready_event")
    if ev is not None:
        ev.record()                                  # materialise the lazy hipEvent_t handle (re-recorded by the library)
    _lib.check(lib.sumk_vasnet_backward_band(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(wts), C.byref(o), _p(dscores), C.byref(g),
                                             _p(dx), _p(ws), ws.numel(), _stream(),
                                             C.c_void_p(ev.cuda_event) if ev is not None else C.c_void_p(0)), "sumk_vasnet_backward_band")
    return dx


# ------------------------------------------------------------------------------------------------ BiLSTM scorers
# SUMK_CHECK=1 (set by the test-suite): synchronise after every recurrent layer and verify that the persistent kernel's
# bounded waits did not time out.  Off by default (it costs a host sync per layer).
CHECK_LSTM = os.environ.get("SUMK_CHECK", "0") == "1"


def _lstm_layer_struct(params, prefix, layer):
    w = _lib.LstmLayerWeights()
    for d, suf in enumerate(("", "_reverse")):
        for f, n in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
            getattr(w, f)[d] = _ptr(params[f"{prefix}{n}_l{layer}{suf}"], f"LSTM weight {prefix}{n}_l{layer}{suf}")
    return w


def bilstm_wplanes(params, prefix, layer, In, H, n_planes, out=None):
    """Weight-plane block of one BiLSTM layer's input projection (sumk_lstm_layer_weights.w_planes), or None when the shape is not eligible."""
    lib = _lib.load()
    nb = lib.sumk_bilstm_wplanes_bytes(int(In), int(H), int(n_planes))
    if nb == 0:
        return None
    w = _lstm_layer_struct(params, prefix, layer)
    view = _aligned_block(nb, params[f"{prefix}weight_ih_l{layer}"].device, out)
    _lib.check(lib.sumk_bilstm_wplanes_build(int(In), int(H), C.byref(w), int(n_planes), _p(view), nb, _stream()), "sumk_bilstm_wplanes_build")
    return view


def bilstm_layer_forward(x, sb, params, prefix, layer, H, training=False, precision=None, wplanes=None, dataset_input=False):
    """x: (n_rows, In) packed -> h (n_rows, 2H) = [h_fwd || h_rev].  Returns (h, workspace or None).
    wplanes (inference in bf16x6 / bf16x3): the layer's weight-plane block -- the input projection then runs on operand planes
    (csrc/gemm_pw.hip); x's planes are kept with the tensor object when dataset_input (layer 0: features), split per call otherwise."""
    lib = _lib.load()
    _check_rows(x, sb, "bilstm input", col="In")
    In = x.shape[1]
    w = _lstm_layer_struct(params, prefix, layer)
    n_planes = PLANES_OF.get(precision)
    xplanes = None
    if wplanes is not None and n_planes and not training and sb.n_rows >= 1024:
        xplanes = (tensor_shadow(x, f"planes{n_planes}", lambda: split_planes(x, n_planes)) if dataset_input and not torch.cuda.is_current_stream_capturing()
                   else split_planes(x, n_planes))
        w.x_planes, w.w_planes = xplanes.data_ptr(), wplanes.data_ptr()
    nbytes = _nonzero(lib.sumk_bilstm_workspace_bytes(In, H, sb.n_seq, sb.off_host_p, int(training)), "sumk_bilstm_workspace_bytes")
    ws = workspace(nbytes, x.device, persistent=training)
    h = torch.empty(sb.n_rows, 2 * H, dtype=torch.float32, device=x.device)
    rc = lib.sumk_bilstm_layer_forward(_p(x), In, H, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(w), _p(h), _p(ws),
                                       ws.numel(), int(training), precision_code(precision), _stream())
    _lib.check(rc, "sumk_bilstm_layer_forward")
    if CHECK_LSTM:
        _lib.check(lib.sumk_bilstm_check(_p(ws), In, H, sb.n_seq, sb.off_host_p, int(training), 0, _stream()), "sumk_bilstm_check")
    return h, (ws if training else None)


def health_check():
    """Raises SumkError if a persistent recurrence kernel on the current device timed out since the last check (its
    outputs, and everything computed from them, are invalid).  Synchronises the current stream; meant for the host
    synchronisation points callers already have (score D2H, per-epoch loss read-back)."""
    _lib.check(_lib.load().sumk_health_check(_stream()), "sumk_health_check")


def mfma_sustained_rate(kind="bf16", iters=4000, random_operands=False):
    """Measurement utility: dense TFLOP/s the current device sustains with nothing but MFMAs in flight (csrc/mfma_probe.hip) -- the practical ceiling of
    an MFMA-bound launch on THIS box, beside the guide's peak.  kind: "bf16" (32x32x16), "f32" (32x32x2), "bf16_16" (16x16x32).  Returns (tflops, seconds)."""
    code = {"bf16": 0, "f32": 1, "bf16_16": 2}[kind] + (4 if random_operands else 0)
    t, sec = C.c_double(0.0), C.c_double(0.0)
    _lib.check(_lib.load().sumk_probe_mfma_rate(code, int(iters), C.byref(t), C.byref(sec), _stream()), "sumk_probe_mfma_rate")
    return t.value, sec.value


def frame_head_forward(h, w, b):
    """scores = sigmoid(h @ w.T + b) for h (n_rows, F), w (1, F) or (F,), b (1,)."""
    lib = _lib.load()
    _require_gpu(h, "frame head input")
    scores = torch.empty(h.shape[0], dtype=torch.float32, device=h.device)
    rc = lib.sumk_frame_head_forward(_p(h), h.shape[0], h.shape[1], _p(w), _p(b), _p(scores), _stream())
    _lib.check(rc, "sumk_frame_head_forward")
    return scores


# ------------------------------------------------------------------------------------------------ training
def vasnet_backward_packed(x, sb, params, opts, dscores, ws, grads, want_dx=False):
    """Accumulates d(sum dscores*scores)/d(weights) into `grads` (dict state_dict-key -> preallocated tensor)."""
    lib = _lib.load()
    D = x.shape[1]
    w, o = _vasnet_structs(params, opts)
    g = _lib.VasnetGrads()
    for f, k in VASNET_FIELDS:
        t = grads[k]
        _require_gpu(t, f"VASNet grad {k}")
        setattr(g, f, t.data_ptr())
    dx = torch.empty_like(x) if want_dx else None
    if not dscores.is_contiguous():
        dscores = dscores.contiguous()
    ev = opts.get("tail_grads_ready_event")          # torch.cuda.Event recorded mid-backward (data-parallel overlap) or None
    if ev is not None:
        ev.record()                                  # materialise the lazy hipEvent_t handle (re-recorded by the library)
    rc = lib.sumk_vasnet_backward(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(w), C.byref(o), _p(dscores),
                                  C.byref(g), _p(dx), _p(ws), ws.numel(), _stream(),
                                  C.c_void_p(ev.cuda_event) if ev is not None else C.c_void_p(0))
    _lib.check(rc, "sumk_vasnet_backward")
    return dx


# Bumped by every C-ABI call that WRITES model weights (the optimiser kernels): torch cannot see those writes (no ._version bump,
# same storage), so caches derived from weights -- VASNet's folded Wvo -- carry this counter in their key.
WEIGHTS_EPOCH = [0]


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """In-place torch.optim.Adam-equivalent update of one flat fp32 buffer (HIP kernel)."""
    lib = _lib.load()
    for t in (param, grad, exp_avg, exp_avg_sq):
        _require_gpu(t, "adam_step")
        if not t.is_contiguous():
            raise SumkError("adam_step: buffers must be contiguous")
    rc = lib.sumk_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, betas[0], betas[1], eps,
                            weight_decay, int(step), float(grad_scale), _stream())
    _lib.check(rc, "sumk_adam_step")
    WEIGHTS_EPOCH[0] += 1


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, state, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                  sumsq=None, max_norm=0.0, zero_grad=False):
    """The same update with the step counter (state[0], int32, incremented by the call) and, when `sumsq` (device scalar, squared
    L2 norm of the unscaled gradient) is given, the clip_grad_norm_ coefficient kept ON THE DEVICE: no host sync, capturable into
    a HIP graph.  `state`: 4 x int32 device block, zeroed once by the owner."""
    lib = _lib.load()
    for t in (param, grad, exp_avg, exp_avg_sq):
        _require_gpu(t, "adam_step_dev")
        if not t.is_contiguous():
            raise SumkError("adam_step_dev: buffers must be contiguous")
    if not state.is_cuda or state.dtype != torch.int32 or state.numel() < 4 or not state.is_contiguous():
        raise SumkError("adam_step_dev: state must be a contiguous int32 GPU tensor of 4 elements")
    fn = lib.sumk_adam_step_dev_zero_grad if zero_grad else lib.sumk_adam_step_dev      # zero_grad: the gradient buffer is left zero
    rc = fn(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, betas[0], betas[1], eps,
            weight_decay, _p(state), float(grad_scale), None if sumsq is None else _p(sumsq), float(max_norm), _stream())
    _lib.check(rc, "sumk_adam_step_dev")
    WEIGHTS_EPOCH[0] += 1


def cast_f32_bf16(src, dst):
    """dst (bf16, same numel) <- src (fp32), round to nearest even (HIP)."""
    _require_gpu(src, "cast_f32_bf16")
    if dst.dtype != torch.bfloat16 or dst.numel() != src.numel() or not (src.is_contiguous() and dst.is_contiguous()):
        raise SumkError("cast_f32_bf16: dst must be a contiguous bfloat16 buffer of the same size")
    _lib.check(_lib.load().sumk_cast_f32_bf16(_p(src), _p(dst), src.numel(), _stream()), "sumk_cast_f32_bf16")


def cast_bf16_f32(src, dst):
    """dst (fp32) <- src (bf16) (HIP)."""
    _require_gpu(dst, "cast_bf16_f32")
    if src.dtype != torch.bfloat16 or dst.numel() != src.numel() or not (src.is_contiguous() and dst.is_contiguous()):
        raise SumkError("cast_bf16_f32: src must be a contiguous bfloat16 buffer of the same size")
    _lib.check(_lib.load().sumk_cast_bf16_f32(_p(src), _p(dst), src.numel(), _stream()), "sumk_cast_bf16_f32")


_sumsq_ws = {}


def sumsq(v, out=None):
    """out[0] += sum(v*v) (HIP, deterministic).  Returns the 1-element device tensor."""
    lib = _lib.load()
    _require_gpu(v, "sumsq")
    if out is None:
        out = torch.zeros(1, dtype=torch.float32, device=v.device)
    ws = _sumsq_ws.get(str(v.device))
    if ws is None:
        ws = _sumsq_ws[str(v.device)] = torch.empty(lib.sumk_sumsq_workspace_bytes(), dtype=torch.uint8, device=v.device)
    _lib.check(lib.sumk_sumsq(_p(v), v.numel(), _p(out), _p(ws), _stream()), "sumk_sumsq")
    return out


def logistic_step_workspace_bytes(n_rows, D):
    return int(_lib.load().sumk_logistic_step_workspace_bytes(int(n_rows), int(D)))


def logistic_step(x, sb, target, flat_param, flat_grad, exp_avg, exp_avg_sq, state, lr, betas=(0.9, 0.999), eps=1e-8,
                  weight_decay=0.0, scale=1.0, apply_adam=True, want_scores=False, loss=None, mse=None, scores=None, ws=None):
    """One optimiser step of the logistic baseline in one launch (sumk_logistic_step, csrc/logistic.hip) on FlatAdam-shaped buckets
    ([w (D) | b | padding], D + 4 floats each).  apply_adam: torch's Adam applied in the kernel (state: FlatAdam._state, incremented);
    otherwise [dW | db] is added to flat_grad.  Returns (loss (1,), mse per video (n_seq,), scores (n_rows,) or None), all on the device.
    loss / mse / scores / ws: caller-owned outputs and workspace (a captured step keeps fixed addresses); allocated when None."""
    lib = _lib.load()
    _require_gpu(x, "logistic_step x"); _require_gpu(target, "logistic_step target")
    n_rows, D = x.shape
    if n_rows != sb.n_rows or target.shape != (sb.n_rows,):
        raise SumkError(f"logistic_step: x {tuple(x.shape)} / target {tuple(target.shape)} do not fit {sb.n_rows} rows")
    bufs = (flat_param, flat_grad) if not apply_adam else (flat_param, exp_avg, exp_avg_sq)
    for t in bufs:
        _require_gpu(t, "logistic_step bucket")
        if t.numel() < D + 4 or not t.is_contiguous():
            raise SumkError(f"logistic_step: flat buckets must be contiguous with >= D + 4 = {D + 4} floats, got {t.numel()}")
    if apply_adam and (not state.is_cuda or state.dtype != torch.int32 or state.numel() < 4):
        raise SumkError("logistic_step: state must be an int32 GPU tensor of 4 elements")
    dev = x.device
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    if mse is None:
        mse = torch.empty(sb.n_seq, dtype=torch.float32, device=dev)
    if want_scores and scores is None:
        scores = torch.empty(n_rows, dtype=torch.float32, device=dev)
    nb = lib.sumk_logistic_step_workspace_bytes(n_rows, D)
    if ws is None:
        ws = workspace(nb, dev)
    rc = lib.sumk_logistic_step(_p(x.contiguous()), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, _p(target.contiguous()), _p(flat_param),
                                _p(flat_grad), _p(exp_avg), _p(exp_avg_sq), _p(state), float(lr), float(betas[0]), float(betas[1]),
                                float(eps), float(weight_decay), float(scale), 1 if apply_adam else 0, _p(loss), _p(mse), _p(scores),
                                _p(ws), ws.numel(), _stream())
    _lib.check(rc, "sumk_logistic_step")
    if apply_adam:
        WEIGHTS_EPOCH[0] += 1
    return loss, mse, scores


def bilstm_layer_backward(x, h, dh, sb, params, grads, prefix, layer, H, ws, want_dx, precision=None, tail_event=None):
    """BPTT of one bidirectional layer; accumulates into grads[<prefix>{weight,bias}_{ih,hh}_l{layer}[_reverse]].
    tail_event (torch.cuda.Event, data-parallel trainers): recorded by the library once the biases' and the reverse direction's gradients
    are final, before the forward direction's weight-gradient GEMMs (sumk_lstm_layer_grads.tail_ready_event)."""
    lib = _lib.load()
    In = x.shape[1]
    w = _lstm_layer_struct(params, prefix, layer)
    g = _lib.LstmLayerGrads()
    for d, suf in enumerate(("", "_reverse")):
        for f, n in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
            getattr(g, f)[d] = grads[f"{prefix}{n}_l{layer}{suf}"].data_ptr()
    if tail_event is not None:
        tail_event.record()                          # materialise the lazy hipEvent_t handle (re-recorded by the library)
        g.tail_ready_event = tail_event.cuda_event
    dx = torch.empty_like(x) if want_dx else None
    if not dh.is_contiguous():
        dh = dh.contiguous()
    rc = lib.sumk_bilstm_layer_backward(_p(x), _p(h), _p(dh), In, H, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(w),
                                        C.byref(g), _p(dx), _p(ws), ws.numel(), precision_code(precision), _stream())
    _lib.check(rc, "sumk_bilstm_layer_backward")
    if CHECK_LSTM:
        _lib.check(lib.sumk_bilstm_check(_p(ws), In, H, sb.n_seq, sb.off_host_p, 1, 1, _stream()), "sumk_bilstm_check")
    return dx


def frame_head_backward(h, scores, dscores, w, dw, db):
    lib = _lib.load()
    F = h.shape[1]
    nb = lib.sumk_frame_head_workspace_bytes(F)
    ws = torch.empty(nb, dtype=torch.uint8, device=h.device)
    dh = torch.empty_like(h)
    if not dscores.is_contiguous():
        dscores = dscores.contiguous()
    rc = lib.sumk_frame_head_backward(_p(h), _p(scores), _p(dscores), h.shape[0], F, _p(w), _p(dh), _p(dw), _p(db), _p(ws),
                                      nb, _stream())
    _lib.check(rc, "sumk_frame_head_backward")
    return dh


# ------------------------------------------------------------------------------------------------ DSN reward
REWARD_PATHS = ("gram", "stream")
REWARD_STREAM_EC = 8       # episodes per pass of the streaming reward (include/sumk.h: SUMK_REWARD_STREAM_EC)


def _reward_path(path):
    if path not in REWARD_PATHS:
        raise SumkError(f"dsn_reward: path must be one of {REWARD_PATHS}, got {path!r}")
    return path


def dsn_reward_workspace_bytes(D, sb, E, path="gram"):
    """Bytes of scratch one dsn_reward call takes: O(sum T^2) on the "gram" path, O(E * n_rows) on the "stream" path."""
    lib = _lib.load()
    name = "sumk_dsn_reward_workspace_bytes" if _reward_path(path) == "gram" else "sumk_dsn_reward_stream_workspace_bytes"
    return _nonzero(getattr(lib, name)(int(D), sb.n_seq, sb.off_host_p, int(E)), name)


def dsn_reward_stream_plan(sb):
    """The column split count that col_split=0 stands for on the "stream" path."""
    return int(_lib.load().sumk_dsn_reward_stream_plan(sb.n_seq, sb.off_host_p))


def dsn_reward(x, sb, actions, far_sim=False, temp_dist_thre=20, path="gram", col_split=0):
    """actions: (E, n_rows) 0/1 floats -> rewards (E, n_seq) (dsn.py:185-236) for a packed batch.
    path="gram": one Gram matrix per video in the workspace (csrc/reward.hip); path="stream": the Gram tiles are consumed in registers
    (csrc/reward_stream.hip; videos of up to 1 048 576 frames), col_split forces the number of column splits (0: the library's plan)."""
    lib = _lib.load()
    _reward_path(path)
    _require_gpu(x, "dsn_reward features"); _require_gpu(actions, "dsn_reward actions")
    E = actions.shape[0]
    if actions.dim() != 2 or actions.shape[1] != sb.n_rows or not actions.is_contiguous():
        raise SumkError(f"dsn_reward: actions must be contiguous (E, {sb.n_rows}), got {tuple(actions.shape)}")
    D = x.shape[1]
    if path == "stream":
        _check_rows(x, sb, "dsn_reward features")
        nb = dsn_reward_workspace_bytes(D, sb, E, "stream")
        ws = workspace(nb, x.device)
        out = torch.empty(E, sb.n_seq, dtype=torch.float32, device=x.device)
        rc = lib.sumk_dsn_reward_stream(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, _p(actions), E, int(bool(far_sim)),
                                        int(temp_dist_thre), int(col_split), _p(out), _p(ws), ws.numel(), _stream())
        _lib.check(rc, "sumk_dsn_reward_stream")
        return out
    nb = _nonzero(lib.sumk_dsn_reward_workspace_bytes(D, sb.n_seq, sb.off_host_p, E), "sumk_dsn_reward_workspace_bytes")
    ws = workspace(nb, x.device)
    out = torch.empty(E, sb.n_seq, dtype=torch.float32, device=x.device)
    rc = lib.sumk_dsn_reward(_p(x), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, _p(actions), E, int(bool(far_sim)),
                             int(temp_dist_thre), _p(out), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "sumk_dsn_reward")
    return out


# ------------------------------------------------------------------------------------------------ change points (KTS)
KTS_MAX_STEPS = 16384      # per video: sumk_kts (include/sumk.h)


def kts_workspace_bytes(D, sb, max_ncp):
    return _lib.load().sumk_kts_workspace_bytes(int(D), sb.n_seq, sb.off_host_p, int(max_ncp))


def _kts_call(name, src, sb, D, max_ncp, lmin, lmax, vmax, want_scores):
    lib = _lib.load()
    D, max_ncp, lmin, lmax = int(D), int(max_ncp), int(min(lmin, 2 ** 31 - 1)), int(min(lmax, 2 ** 31 - 1))
    if name == "sumk_kts_banded":
        nb = _nonzero(lib.sumk_kts_banded_workspace_bytes(D, sb.n_seq, sb.off_host_p, max_ncp, lmax), "sumk_kts_banded_workspace_bytes")
    else:
        nb = _nonzero(lib.sumk_kts_workspace_bytes(D, sb.n_seq, sb.off_host_p, max_ncp), "sumk_kts_workspace_bytes")
    ws = workspace(nb, src.device)
    n_cps = torch.empty(sb.n_seq, dtype=torch.int32, device=src.device)
    cps = torch.empty(sb.n_seq, max(max_ncp, 1), dtype=torch.int32, device=src.device)[:, :max_ncp]
    scores = torch.empty(sb.n_seq, max_ncp + 1, dtype=torch.float64, device=src.device) if want_scores else None
    tail = (_p(n_cps), _p(cps), _p(scores), _p(ws), ws.numel(), _stream())
    if name in ("sumk_kts", "sumk_kts_banded"):
        rc = getattr(lib, name)(_p(src), D, sb.n_seq, sb.off_host_p, sb.off_dev_p, max_ncp, lmin, lmax, float(vmax), *tail)
    elif name == "sumk_kts_gram":
        rc = lib.sumk_kts_gram(_p(src), sb.n_seq, sb.off_host_p, sb.off_dev_p, max_ncp, lmin, lmax, float(vmax), *tail)
    else:
        rc = lib.sumk_kts_gram_nonlin(_p(src), sb.n_seq, sb.off_host_p, sb.off_dev_p, max_ncp, lmin, lmax, *tail)
    _lib.check(rc, name)
    return n_cps, cps, scores


def kts(x, sb, max_ncp, vmax=1.0, lmin=1, lmax=100000, want_scores=True):
    """cpd_auto of every video of a packed batch from its features x (n_rows, D): (n_cps (n_seq,) int32, cps (n_seq, max_ncp) int32 with -1
    behind n_cps[v], scores (n_seq, max_ncp + 1) float64 with +inf behind n_cps[v] or None) as device tensors (sumk_kts, include/sumk.h).
    Only enqueues work on the current stream."""
    _require_gpu(x, "kts features")
    if x.dim() != 2 or x.shape[0] != sb.n_rows or not x.is_contiguous():
        raise SumkError(f"kts: features must be contiguous ({sb.n_rows}, D), got {tuple(x.shape)}")
    return _kts_call("sumk_kts", x, sb, x.shape[1], max_ncp, lmin, lmax, vmax, want_scores)


KTS_BANDED_MAX_STEPS = 1048576      # per video: sumk_kts_banded (include/sumk.h)


def kts_banded_workspace_bytes(D, sb, max_ncp, lmax=100000):
    """Bytes sumk_kts_banded needs for this batch: pure host arithmetic, 0 for arguments it would refuse."""
    return _lib.load().sumk_kts_banded_workspace_bytes(int(D), sb.n_seq, sb.off_host_p, int(max_ncp), int(min(lmax, 2 ** 31 - 1)))


def kts_banded(x, sb, max_ncp, vmax=1.0, lmin=1, lmax=100000, want_scores=True):
    """`kts` for long videos: only the band J[t, t .. t + min(lmax, n) - 1] is kept and every row of the dynamic programme is one launch
    over the whole chip (sumk_kts_banded, include/sumk.h).  Same outputs, bit for bit, wherever `kts` accepts the input.  Only enqueues
    work on the current stream."""
    _require_gpu(x, "kts_banded features")
    if x.dim() != 2 or x.shape[0] != sb.n_rows or not x.is_contiguous():
        raise SumkError(f"kts_banded: features must be contiguous ({sb.n_rows}, D), got {tuple(x.shape)}")
    return _kts_call("sumk_kts_banded", x, sb, x.shape[1], max_ncp, lmin, lmax, vmax, want_scores)


def _kts_gram_check(K, sb):
    want = sum(n * n for n in sb.lens)
    if not K.is_cuda or K.dtype != torch.float64 or K.dim() != 1 or K.numel() != want or not K.is_contiguous():
        raise SumkError(f"kts_gram: expected a flat contiguous float64 GPU tensor of {want} elements ((n x n) blocks back to back), got "
                        f"{K.dtype} {tuple(K.shape)} on {K.device}")


def kts_gram(K, sb, max_ncp, vmax=1.0, lmin=1, lmax=100000, want_scores=True):
    """The same from the caller's float64 kernel matrices: K is flat, the (n_v x n_v) blocks back to back (sumk_kts_gram)."""
    _kts_gram_check(K, sb)
    return _kts_call("sumk_kts_gram", K, sb, 4, max_ncp, lmin, lmax, vmax, want_scores)


def kts_gram_nonlin(K, sb, ncp, lmin=1, lmax=100000, want_scores=True):
    """cpd_nonlin: the fixed-m backtrack from row min(ncp, n - 1), no penalty; scores = the whole row I[., n] (sumk_kts_gram_nonlin)."""
    _kts_gram_check(K, sb)
    return _kts_call("sumk_kts_gram_nonlin", K, sb, 4, ncp, lmin, lmax, 1.0, want_scores)


def kts_segments(n_cps, cps, sb, picks_ptrs, n_frames):
    """(n_cps, cps) of `kts` -> (change_points (n_seq, max_ncp + 1, 2), n_frame_per_seg (n_seq, max_ncp + 1)) int32 device tensors, the
    layout the evaluation tail reads, padded with empty segments behind n_cps[v] + 1 (sumk_kts_segments, include/sumk.h).
    picks_ptrs: (n_seq,) int64 device tensor of device pointers to each video's int32 picks (0: the identity), or None; n_frames: (n_seq,)
    int32 device tensor.  Only enqueues work on the current stream."""
    max_ncp = int(cps.shape[1])
    change_points = torch.empty(sb.n_seq, max_ncp + 1, 2, dtype=torch.int32, device=cps.device)
    nfps = torch.empty(sb.n_seq, max_ncp + 1, dtype=torch.int32, device=cps.device)
    _lib.check(_lib.load().sumk_kts_segments(_p(n_cps), _p(cps), sb.n_seq, max_ncp, sb.off_dev_p, _p(picks_ptrs), _p(n_frames), _p(change_points),
                                             _p(nfps), _stream()), "sumk_kts_segments")
    return change_points, nfps


def eval_segments_long(scores, descr_dev, descr_host, frame_scratch, seg_means):
    """Upsample + float32 segment means for videos past the 4096 picks of the one-workgroup tail (sumk_eval_device_segments_long,
    include/sumk.h).  descr_host: a ctypes array of _lib.EvalDevVideo, descr_dev: its bytes as a device tensor.  Only enqueues work."""
    _lib.check(_lib.load().sumk_eval_device_segments_long(_p(scores), _p(descr_dev), C.cast(descr_host, C.c_void_p), len(descr_host), _p(frame_scratch),
                                                          _p(seg_means), _stream()), "sumk_eval_device_segments_long")


def eval_select_long_workspace_bytes(n_videos, max_n_segs, max_capacity):
    return _nonzero(_lib.load().sumk_eval_device_select_long_workspace_bytes(int(n_videos), int(max_n_segs), int(max_capacity)),
                    "sumk_eval_device_select_long_workspace_bytes")


def eval_select_long(descr_dev, descr_host, summary, selected, f_avg, f_max, status, ws):
    """Key shots, expanded summaries and F-scores at any frame budget (sumk_eval_device_select_long, include/sumk.h).  descr_host: a ctypes
    array of _lib.EvalDevSelect, descr_dev: its bytes as a device tensor; ws: eval_select_long_workspace_bytes(...) bytes.  Only enqueues work."""
    _lib.check(_lib.load().sumk_eval_device_select_long(_p(descr_dev), C.cast(descr_host, C.c_void_p), len(descr_host), _p(summary), summary.numel(),
                                                        _p(selected), selected.numel(), _p(f_avg), _p(f_max), _p(status), _p(ws), ws.numel(), _stream()),
               "sumk_eval_device_select_long")


def eval_spearman_long_workspace_bytes(descr_host):
    """Workspace of eval_spearman_long for these videos (a ctypes array of _lib.EvalDevVideo); pure host arithmetic."""
    return _nonzero(_lib.load().sumk_eval_device_spearman_long_workspace_bytes(C.cast(descr_host, C.c_void_p), len(descr_host)),
                    "sumk_eval_device_spearman_long_workspace_bytes")


def eval_spearman_long(scores, descr_dev, descr_host, ws, corr):
    """Mean Spearman correlation per video for any number of picks and frames the long tail accepts (sumk_eval_device_spearman_long,
    include/sumk.h), into corr (n_videos,) float64.  ws: eval_spearman_long_workspace_bytes(descr_host) bytes.  Only enqueues work."""
    _lib.check(_lib.load().sumk_eval_device_spearman_long(_p(scores), _p(descr_dev), C.cast(descr_host, C.c_void_p), len(descr_host), _p(ws), ws.numel(),
                                                          _p(corr), _stream()), "sumk_eval_device_spearman_long")


def eval_kendall_long_workspace_bytes(descr_host):
    """Workspace of eval_kendall_long for these videos (a ctypes array of _lib.EvalDevVideo); pure host arithmetic."""
    return _nonzero(_lib.load().sumk_eval_device_kendall_long_workspace_bytes(C.cast(descr_host, C.c_void_p), len(descr_host)),
                    "sumk_eval_device_kendall_long_workspace_bytes")


def eval_kendall_long(scores, descr_dev, descr_host, kendall_dev, ws, corr, counts=None):
    """Mean Kendall tau-b per video, and (counts given: (sum n_users, 4) int64) the pair counts {cmd, xtie, ytie, ntie}, for any number of
    picks and frames the long tail accepts (sumk_eval_device_kendall_long, include/sumk.h).  kendall_dev: the bytes of a ctypes array of
    _lib.EvalDevKendall as a device tensor; ws: eval_kendall_long_workspace_bytes(descr_host) bytes.  Only enqueues work."""
    _lib.check(_lib.load().sumk_eval_device_kendall_long(_p(scores), _p(descr_dev), C.cast(descr_host, C.c_void_p), _p(kendall_dev), len(descr_host),
                                                         _p(ws), ws.numel(), _p(corr), _p(counts), _stream()), "sumk_eval_device_kendall_long")


def dsn_policy_loss_forward(probs, sb, actions, rewards, base, beta, eps_target):
    """(loss_per_video (n_seq,), mean_probs (n_seq,)) of sumk_dsn_policy_loss_forward (include/sumk.h)."""
    lib = _lib.load()
    for t, what in ((probs, "probs"), (actions, "actions"), (rewards, "rewards"), (base, "base")):
        _require_gpu(t, "dsn_policy_loss " + what)
        if not t.is_contiguous():
            raise SumkError(f"dsn_policy_loss: {what} must be contiguous")
    E = actions.shape[0]
    if probs.shape != (sb.n_rows,) or actions.shape != (E, sb.n_rows) or rewards.shape != (E, sb.n_seq) or base.shape != (sb.n_seq,):
        raise SumkError(f"dsn_policy_loss: shapes probs {tuple(probs.shape)} actions {tuple(actions.shape)} rewards "
                        f"{tuple(rewards.shape)} base {tuple(base.shape)} do not fit {sb.n_rows} rows / {sb.n_seq} videos")
    lv = torch.empty(sb.n_seq, dtype=torch.float32, device=probs.device)
    mp = torch.empty(sb.n_seq, dtype=torch.float32, device=probs.device)
    rc = lib.sumk_dsn_policy_loss_forward(_p(probs), _p(actions), _p(rewards), _p(base), sb.n_seq, sb.n_rows, sb.off_dev_p, E,
                                          float(beta), float(eps_target), _p(lv), _p(mp), _stream())
    _lib.check(rc, "sumk_dsn_policy_loss_forward")
    return lv, mp


def dsn_policy_loss_backward(probs, sb, actions, rewards, base, mean_probs, dlv, beta, eps_target):
    lib = _lib.load()
    dlv = dlv.contiguous()
    dprobs = torch.empty_like(probs)
    rc = lib.sumk_dsn_policy_loss_backward(_p(probs), _p(actions), _p(rewards), _p(base), _p(mean_probs), _p(dlv), sb.n_seq, sb.n_rows,
                                           sb.off_dev_p, actions.shape[0], float(beta), float(eps_target), _p(dprobs), _stream())
    _lib.check(rc, "sumk_dsn_policy_loss_backward")
    return dprobs


# ------------------------------------------------------------------------------------------------ Transformer scorer
TF_LAYER_FIELDS = (("in_proj_w", "self_attn.in_proj_weight"), ("in_proj_b", "self_attn.in_proj_bias"),
                   ("out_proj_w", "self_attn.out_proj.weight"), ("out_proj_b", "self_attn.out_proj.bias"),
                   ("lin1_w", "linear1.weight"), ("lin1_b", "linear1.bias"), ("lin2_w", "linear2.weight"),
                   ("lin2_b", "linear2.bias"), ("norm1_w", "norm1.weight"), ("norm1_b", "norm1.bias"),
                   ("norm2_w", "norm2.weight"), ("norm2_b", "norm2.bias"))
TF_HEAD_FIELDS = (("ln_w", "layer_norm.weight"), ("ln_b", "layer_norm.bias"), ("k1_w", "k1.weight"), ("k1_b", "k1.bias"),
                  ("k2_w", "k2.weight"), ("k2_b", "k2.bias"))


def transformer_param_names(n_layers):
    """state_dict keys the HIP path reads (the prototype `transformer_encoder_layer.*` copy is never used)."""
    names = [f"transformer_encoder.layers.{l}.{k}" for l in range(n_layers) for _, k in TF_LAYER_FIELDS]
    return names + [k for _, k in TF_HEAD_FIELDS]


def _tf_structs(tensors, n_layers, what, layer_cls, head_cls):
    def ptr(k):
        return _ptr(tensors[k], f"Transformer {what} {k}")
    layers = (layer_cls * n_layers)()
    for l in range(n_layers):
        for f, k in TF_LAYER_FIELDS:
            setattr(layers[l], f, ptr(f"transformer_encoder.layers.{l}.{k}"))
    head = head_cls(*[ptr(k) for _, k in TF_HEAD_FIELDS])
    return layers, head


def _tf_opts(o):
    wp = o.get("wplanes")
    return _lib.TfOpts(float(o["layer_eps"]), float(o["final_eps"]), int(bool(o.get("more_residuals", False))),
                       float(o.get("layer_dropout_p", 0.0)), float(o.get("head_dropout_p", 0.0)), int(o.get("seed", 0)),
                       precision_code(o.get("precision")), wp.data_ptr() if wp is not None else None)


def transformer_wplanes(params, D, dff, n_layers, n_planes, out=None):
    """The weight-plane block of the Transformer scorer's plane path (sumk_tf_opts.wplanes) for the current weights: planes of in_proj,
    out_proj, linear1, linear2 of every layer and of k1.  Returns a 256-byte aligned uint8 tensor, or None when (D, dff) is not eligible."""
    lib = _lib.load()
    nb = lib.sumk_transformer_wplanes_bytes(int(D), int(dff), int(n_layers), int(n_planes))
    if nb == 0:
        return None
    layers, head = _tf_structs(params, n_layers, "weight", _lib.TfLayerWeights, _lib.TfHeadWeights)
    view = _aligned_block(nb, params[TF_HEAD_FIELDS[0][1]].device, out)
    _lib.check(lib.sumk_transformer_wplanes_build(int(D), int(dff), int(n_layers), C.cast(layers, C.c_void_p), C.cast(C.pointer(head), C.c_void_p),
                                                  int(n_planes), _p(view), nb, _stream()), "sumk_transformer_wplanes_build")
    return view


TF_ATTENTION = ("dense", "stream")
TF_ATTENTION_PRECISION = ("fp32", "bf16x3")     # arithmetic of the attention products on "stream" (scoring)


def _tf_attention(attention):
    if attention not in TF_ATTENTION:
        raise SumkError(f"transformer: attention must be one of {TF_ATTENTION}, got {attention!r}")
    return attention


_TfPath = collections.namedtuple("_TfPath", "query forward backward code persistent")


def _tf_path(attention, attention_precision="fp32", attention_train_precision="fp32", training=False):
    """The library path of one scorer call: the entries of its size query, forward and backward (None outside training), the precision
    code the bf16x3 stream entries take (None: the path has no such argument) and whether the workspace outlives the call (the training
    forward's goes to the backward).  attention_precision="bf16x3" is scoring on "stream" only, attention_train_precision="bf16x3"
    training on "stream" only."""
    code = _stream_precision(attention_precision, "transformer attention")
    if code is not None and (_tf_attention(attention) != "stream" or training):
        raise SumkError(f"transformer: attention_precision={attention_precision!r} needs attention=\"stream\" and training=False")
    tcode = _stream_precision(attention_train_precision, "transformer attention (training)")
    if tcode is not None and (_tf_attention(attention) != "stream" or not training):
        raise SumkError(f"transformer: attention_train_precision={attention_train_precision!r} needs attention=\"stream\" and training=True")
    if _tf_attention(attention) == "dense":
        return _TfPath("sumk_transformer_workspace_bytes_for", "sumk_transformer_forward", "sumk_transformer_backward" if training else None,
                       None, bool(training))
    code = tcode if training else code
    split, train = "_split" if code is not None else "", "_train" if training else ""
    return _TfPath(f"sumk_transformer_stream{split}{train}_workspace_bytes", f"sumk_transformer_forward_stream{split}{train}",
                   f"sumk_transformer_backward_stream{split}" if training else None, code, bool(training))


def attn_strips_b16_sizes(sb):
    """(elements of E, elements of P16) the bf16 attention strips address for a batch (sumk_attn_strips_b16_sizes; host arithmetic)."""
    e, p = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().sumk_attn_strips_b16_sizes(sb.n_seq, sb.off_host_p, C.byref(e), C.byref(p)), "sumk_attn_strips_b16_sizes")
    return e.value, p.value


def attn_strips_b16(backward, a, b, c, out, E, P16, sb, scale, ignore_self=False, aperture=-1, dropout_p=0.0, seed=0):
    """The fused attention strips of the bf16 training step on their own (csrc/attn_b16.hip through sumk_attn_strips_b16: TESTS AND PROBES,
    the call synchronises).  a, b, c, out: bfloat16 (n_rows, D) with unit column stride, any row stride (slices of one buffer are fine);
    E: float32, P16: bfloat16, both flat and caller-owned, at least attn_strips_b16_sizes(sb) elements.
    Forward: a, b, c = Q, K, V; writes E (alpha), P16 (bf16 dropout(alpha)), out (CTX).  Backward: a, b, c = dCTX, V, K; reads E, writes
    P16 (bf16 dS) and out (dQ)."""
    lib = _lib.load()
    for t, what in ((a, "a"), (b, "b"), (c, "c"), (out, "out")):
        if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 2 or t.shape != a.shape or t.shape[0] != sb.n_rows or t.stride(1) != 1:
            raise SumkError(f"attn_strips_b16: {what} must be a GPU bfloat16 (n_rows={sb.n_rows}, D) tensor with unit column stride, got "
                            f"{t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    ne, np16 = attn_strips_b16_sizes(sb)
    if not E.is_cuda or E.dtype != torch.float32 or not E.is_contiguous() or E.numel() < ne:
        raise SumkError(f"attn_strips_b16: E must be a contiguous GPU float32 tensor of at least {ne} elements")
    if not P16.is_cuda or P16.dtype != torch.bfloat16 or not P16.is_contiguous() or P16.numel() < np16:
        raise SumkError(f"attn_strips_b16: P16 must be a contiguous GPU bfloat16 tensor of at least {np16} elements")
    rc = lib.sumk_attn_strips_b16(int(bool(backward)), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
                                  out.data_ptr(), out.stride(0), E.data_ptr(), P16.data_ptr(), a.shape[1], sb.n_seq, sb.off_host_p,
                                  float(scale), int(bool(ignore_self)), int(aperture), float(dropout_p), int(seed), _stream())
    _lib.check(rc, "sumk_attn_strips_b16")


def _stream_precision(precision, what):
    """None for "fp32" (the exact stream entries), else the code the bf16x3 stream entries take (they refuse all but "bf16x3")."""
    code = precision_code(precision)
    if code == PRECISIONS["fp32"]:
        return None
    if precision != "bf16x3":
        raise SumkError(f"{what}: precision must be \"fp32\" or \"bf16x3\", got {precision!r}")
    return code


def _attn_stream_entry(suffix, precision, what):
    """(entry, its precision argument as a tuple): sumk_attn_stream<suffix> with nothing for "fp32", sumk_attn_stream_split<suffix> with
    the code for "bf16x3"."""
    code = _stream_precision(precision, what)
    return "sumk_attn_stream" + ("" if code is None else "_split") + suffix, () if code is None else (code,)


def _attn_stream_args(fn, tensors, sb):
    for t, what in tensors:
        _require_gpu(t, f"{fn} {what}")
        if t.dim() != 2 or t.shape != tensors[0][0].shape or t.shape[0] != sb.n_rows or t.stride(1) != 1:
            raise SumkError(f"{fn}: {what} must be (n_rows={sb.n_rows}, D) with unit column stride, got {tuple(t.shape)} strides {t.stride()}")


def attn_stream_workspace_bytes(D, n_heads, sb, precision="fp32"):
    """Bytes of scratch one attn_stream call takes: 16 per video (sumk_attn_stream_workspace_bytes); precision="bf16x3": 24 per video + the
    bf16 planes of Q, K and V, 12 bytes per (padded row, staged column) (sumk_attn_stream_split_workspace_bytes)."""
    entry, code = _attn_stream_entry("_workspace_bytes", precision, "attn_stream")
    return _nonzero(getattr(_lib.load(), entry)(int(D), int(n_heads), sb.n_seq, sb.off_host_p, *code), entry)


def attn_stream(q, k, v, sb, n_heads, scale=None, want_lse=False, precision="fp32"):
    """Multi-head attention of a packed batch without the (T x T) logits (csrc/attn_stream.hip; exact fp32, no mask): q, k, v are (n_rows, D)
    float32, each with unit column stride and any row stride >= D that is a multiple of 4 -- three buffers, or the column slices of one
    (n_rows, 3 D) [Q | K | V] buffer; head h is columns [h D / n_heads, (h + 1) D / n_heads).  scale: None = 1 / sqrt(D / n_heads); it must
    be positive and finite (the kernel takes a row's maximum before scaling), anything else is refused.
    precision="bf16x3": both products in the split-bf16 arithmetic on the bf16 MFMA (csrc/attn_stream_split.hip; head widths % 8 == 0, up
    to 128); the default keeps the exact call and its bits.
    Returns ctx (n_rows, D), or (ctx, lse (n_rows, n_heads)) with want_lse.  Only enqueues work."""
    entry, code = _attn_stream_entry("", precision, "attn_stream")
    _attn_stream_args("attn_stream", ((q, "q"), (k, "k"), (v, "v")), sb)
    D = q.shape[1]
    ws = workspace(attn_stream_workspace_bytes(D, n_heads, sb, precision), q.device)
    ctx = torch.empty(sb.n_rows, D, dtype=torch.float32, device=q.device)
    lse = torch.empty(sb.n_rows, int(n_heads), dtype=torch.float32, device=q.device) if want_lse else None
    sc = 1.0 / math.sqrt(D // int(n_heads)) if scale is None else float(scale)
    rc = getattr(_lib.load(), entry)(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), D, int(n_heads), sb.n_seq, sb.off_host_p,
                                     sb.off_dev_p, sc, *code, _p(ctx), D, _p(lse), _p(ws), ws.numel(), _stream())
    _lib.check(rc, entry)
    return (ctx, lse) if want_lse else ctx


def attn_stream_train(q, k, v, sb, n_heads, scale=None, dropout_p=0.0, seed=0, site=0, precision="fp32"):
    """attn_stream in its training form (sumk_attn_stream_train): the weights dropped with probability dropout_p by the library's hash masks
    of (seed, site) -- the masks the dense Transformer path draws at that site -- and, for attn_stream_backward, stats (n_rows, n_heads, 2):
    the row maximum of the scaled logits and the sum of exp(s - max).  With dropout_p == 0 ctx has attn_stream's bits.
    precision="bf16x3": both products in the split-bf16 arithmetic (sumk_attn_stream_split_train; head widths % 8 == 0, up to 128; same
    masks); the default keeps the exact call and its bits.
    Returns (ctx, stats).  Only enqueues work."""
    entry, code = _attn_stream_entry("_train", precision, "attn_stream_train")
    _attn_stream_args("attn_stream_train", ((q, "q"), (k, "k"), (v, "v")), sb)
    D = q.shape[1]
    ws = workspace(attn_stream_workspace_bytes(D, n_heads, sb, precision), q.device)
    ctx = torch.empty(sb.n_rows, D, dtype=torch.float32, device=q.device)
    stats = torch.empty(sb.n_rows, int(n_heads), 2, dtype=torch.float32, device=q.device)
    sc = 1.0 / math.sqrt(D // int(n_heads)) if scale is None else float(scale)
    rc = getattr(_lib.load(), entry)(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), D, int(n_heads), sb.n_seq, sb.off_host_p,
                                     sb.off_dev_p, sc, float(dropout_p), int(seed), int(site), _p(ctx), D, _p(stats), _p(ws), ws.numel(),
                                     _stream(), *code)
    _lib.check(rc, entry)
    return ctx, stats


def attn_stream_backward_workspace_bytes(D, n_heads, sb, precision="fp32"):
    """Bytes of scratch one attn_stream_backward call takes: 16 per video + 4 per (row, head); precision="bf16x3": 24 per video + 4 per (row,
    head) + the bf16 planes of Q, K, V and dctx, 28 bytes per (padded row, staged column)."""
    entry, code = _attn_stream_entry("_backward_workspace_bytes", precision, "attn_stream_backward")
    return _nonzero(getattr(_lib.load(), entry)(int(D), int(n_heads), sb.n_seq, sb.off_host_p, *code), entry)


def attn_stream_backward(q, k, v, ctx, dctx, stats, sb, n_heads, scale=None, dropout_p=0.0, seed=0, site=0, out=None, precision="fp32", ws=None):
    """Backward of attn_stream_train without anything of size T x T (csrc/attn_stream_bwd.hip; head widths up to 128): ctx and stats are that
    call's results, scale / dropout_p / seed / site its arguments.  Returns (dq, dk, dv), each (n_rows, D) -- the column blocks of one
    (n_rows, 3 D) buffer, `out` when given.  precision="bf16x3": the seven products in the split-bf16 arithmetic
    (csrc/attn_stream_split_bwd.hip).  ws: a uint8 scratch tensor of at least attn_stream_backward_workspace_bytes, else the shared one.
    Deterministic; only enqueues work."""
    entry, code = _attn_stream_entry("_backward", precision, "attn_stream_backward")
    _attn_stream_args("attn_stream_backward", ((q, "q"), (k, "k"), (v, "v"), (ctx, "ctx"), (dctx, "dctx")), sb)
    D = q.shape[1]
    _require_gpu(stats, "attn_stream_backward stats")
    if tuple(stats.shape) != (sb.n_rows, int(n_heads), 2) or not stats.is_contiguous():
        raise SumkError(f"attn_stream_backward: stats must be contiguous (n_rows={sb.n_rows}, n_heads={int(n_heads)}, 2), got {tuple(stats.shape)}")
    nb = attn_stream_backward_workspace_bytes(D, n_heads, sb, precision)
    if ws is None:
        ws = workspace(nb, q.device)
    elif not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < nb:
        raise SumkError(f"attn_stream_backward: ws must be a contiguous uint8 GPU tensor of at least {nb} bytes")
    if out is None:
        out = torch.empty(sb.n_rows, 3 * D, dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != (sb.n_rows, 3 * D) or not out.is_contiguous():
        raise SumkError(f"attn_stream_backward: out must be contiguous (n_rows={sb.n_rows}, {3 * D}), got {tuple(out.shape)}")
    dq, dk, dv = out[:, :D], out[:, D:2 * D], out[:, 2 * D:]
    sc = 1.0 / math.sqrt(D // int(n_heads)) if scale is None else float(scale)
    rc = getattr(_lib.load(), entry)(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(ctx), ctx.stride(0), _p(dctx),
                                     dctx.stride(0), _p(stats), D, int(n_heads), sb.n_seq, sb.off_host_p, sb.off_dev_p, sc, float(dropout_p),
                                     int(seed), int(site), _p(dq), 3 * D, _p(dk), 3 * D, _p(dv), 3 * D, _p(ws), ws.numel(), _stream(), *code)
    _lib.check(rc, entry)
    return dq, dk, dv


def _tf_workspace_bytes(path, D, dff, n_heads, n_layers, sb, training, plane_precision=0):
    """plane_precision: the dense entry's plane path (scoring in bf16x6 / bf16x3 with the weights' planes given) keeps plane buffers
    behind the carve; 0 elsewhere."""
    extra = (int(training), plane_precision) if path.forward == "sumk_transformer_forward" else () if path.code is None else (path.code,)
    return _nonzero(getattr(_lib.load(), path.query)(int(D), int(dff), int(n_heads), int(n_layers), sb.n_seq, sb.off_host_p, *extra), path.query)


def transformer_workspace_bytes(D, dff, n_heads, n_layers, sb, attention="dense", training=False, attention_precision="fp32",
                                attention_train_precision="fp32"):
    """Bytes of scratch one call takes in exact fp32, from the size query of the call's path (_tf_path).  Scoring: "dense" holds heads x
    T x T logits per video, "stream" none; attention_precision="bf16x3" (scoring on "stream" only): + the bf16 planes of one layer's
    [Q | K | V].  training=True, the forward that keeps what the backward needs: "dense" keeps two heads x T x T blocks per video and
    layer, "stream" 8 bytes per (row, head) and layer; attention_train_precision="bf16x3" (training on "stream" only): + the
    descriptors, delta and planes of one layer's attention backward."""
    path = _tf_path(attention, attention_precision, attention_train_precision, training)
    return _tf_workspace_bytes(path, D, dff, n_heads, n_layers, sb, training)


def transformer_forward_packed(x, sb, params, n_layers, n_heads, dff, opts, pos_table=None, pos_rows=None, training=False,
                               attention="dense", attention_precision="fp32", attention_train_precision="fp32"):
    """x: (n_rows, D) packed -> (scores (n_rows,), workspace or None).  params: state_dict-keyed tensors.  One call of the forward entry
    of the path (_tf_path); with training=True its workspace goes to transformer_backward_packed with the same attention arguments.
    attention="stream" (exact fp32 only): every layer's attention on csrc/attn_stream.hip, no (T x T) logits in the workspace.
    attention_precision="bf16x3" (scoring on "stream" only) / attention_train_precision="bf16x3" (training=True on "stream" only):
    every layer's attention on csrc/attn_stream_split.hip, the projections still exact fp32."""
    lib = _lib.load()
    _check_rows(x, sb, "transformer input")
    D = x.shape[1]
    layers, head = _tf_structs(params, n_layers, "weight", _lib.TfLayerWeights, _lib.TfHeadWeights)
    o = _tf_opts(opts)
    path = _tf_path(attention, attention_precision, attention_train_precision, training)
    dense = path.forward == "sumk_transformer_forward"
    nbytes = _tf_workspace_bytes(path, D, dff, n_heads, n_layers, sb, training, o.precision if dense and o.wplanes else 0)
    ws = workspace(nbytes, x.device, persistent=path.persistent)
    scores = torch.empty(sb.n_rows, dtype=torch.float32, device=x.device)
    code = () if path.code is None else (path.code,)
    mode = (int(training),) if dense else ()
    rc = getattr(lib, path.forward)(_p(x), D, dff, n_heads, n_layers, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.cast(layers, C.c_void_p),
                                    C.cast(C.pointer(head), C.c_void_p), C.cast(C.pointer(o), C.c_void_p), _p(pos_table), _p(pos_rows),
                                    _p(scores), *code, _p(ws), ws.numel(), *mode, _stream())
    _lib.check(rc, path.forward)
    return scores, (ws if path.persistent else None)


def transformer_backward_packed(x, sb, params, grads, n_layers, n_heads, dff, opts, dscores, ws, want_dx=False, attention="dense",
                                attention_train_precision="fp32"):
    """attention, attention_train_precision: those of the training forward that filled `ws`."""
    lib = _lib.load()
    D = x.shape[1]
    layers, head = _tf_structs(params, n_layers, "weight", _lib.TfLayerWeights, _lib.TfHeadWeights)
    glayers, ghead = _tf_structs(grads, n_layers, "grad", _lib.TfLayerWeights, _lib.TfHeadWeights)   # same field layout
    o = _tf_opts(opts)
    dx = torch.empty_like(x) if want_dx else None
    if not dscores.is_contiguous():
        dscores = dscores.contiguous()
    path = _tf_path(attention, attention_train_precision=attention_train_precision, training=True)
    code = () if path.code is None else (path.code,)
    rc = getattr(lib, path.backward)(_p(x), D, dff, n_heads, n_layers, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.cast(layers, C.c_void_p),
                                     C.cast(C.pointer(head), C.c_void_p), C.cast(C.pointer(o), C.c_void_p), _p(dscores),
                                     C.cast(glayers, C.c_void_p), C.cast(C.pointer(ghead), C.c_void_p), _p(dx), *code, _p(ws), ws.numel(),
                                     _stream())
    _lib.check(rc, path.backward)
    return dx


# ------------------------------------------------------------------------------------------------ Transformer stacks (SumGAN-Att)
TF_DEC_LAYER_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                     "multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight",
                     "multihead_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                     "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "norm3.weight", "norm3.bias")   # order of _lib.TF_DEC_LAYER_FIELDS


def tf_encoder_param_names(prefix, n_layers, norm_prefix=None):
    """Keys (under `prefix`, e.g. "transformer_encoder.layers.") the encoder-stack entry reads, layer by layer, then the final norm's."""
    names = [f"{prefix}{l}.{k}" for l in range(n_layers) for _, k in TF_LAYER_FIELDS]
    return names + ([f"{norm_prefix}weight", f"{norm_prefix}bias"] if norm_prefix else [])


def tf_decoder_param_names(prefix, n_layers):
    return [f"{prefix}{l}.{k}" for l in range(n_layers) for k in TF_DEC_LAYER_KEYS]


def _stack_opts(opts):
    o = dict(opts)
    o.setdefault("final_eps", 1e-5)
    return _tf_opts(o)


def _enc_structs(tensors, n_layers):
    """tensors: the encoder-stack's tensors in tf_encoder_param_names order -> (layer array, norm_w, norm_b)"""
    nf = len(TF_LAYER_FIELDS)
    layers = (_lib.TfLayerWeights * n_layers)()
    for l in range(n_layers):
        for i, (f, _) in enumerate(TF_LAYER_FIELDS):
            setattr(layers[l], f, _ptr(tensors[l * nf + i], f"encoder layer {l} {f}"))
    rest = tensors[n_layers * nf:]
    return layers, (tensors_or_none(rest, 0), tensors_or_none(rest, 1))


def tensors_or_none(seq, i):
    return seq[i] if len(seq) > i else None


def tf_encoder_forward(x, sb, tensors, n_layers, n_heads, dff, opts, training=False):
    """Encoder stack (sumk_tf_encoder_forward): x (n_rows, D) packed -> (hidden (n_rows, D), workspace or None).  `tensors` in
    tf_encoder_param_names order; with two trailing tensors the final LayerNorm is applied."""
    lib = _lib.load()
    _check_rows(x, sb, "encoder-stack input")
    D = x.shape[1]
    layers, (nw, nb) = _enc_structs(tensors, n_layers)
    o = _stack_opts(opts)
    nbytes = _nonzero(lib.sumk_tf_encoder_workspace_bytes(D, dff, n_heads, n_layers, sb.n_seq, sb.off_host_p, int(training)), "sumk_tf_encoder_workspace_bytes")
    ws = workspace(nbytes, x.device, persistent=training)
    out = torch.empty_like(x)
    rc = lib.sumk_tf_encoder_forward(_p(x), D, dff, n_heads, n_layers, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.cast(layers, C.c_void_p),
                                     _p(nw), _p(nb), C.cast(C.pointer(o), C.c_void_p), _p(out), _p(ws), ws.numel(), int(training), _stream())
    _lib.check(rc, "sumk_tf_encoder_forward")
    return out, (ws if training else None)


def tf_encoder_backward(x, sb, tensors, grads, n_layers, n_heads, dff, opts, dhidden, ws, want_dx=False):
    """Accumulates into `grads` (same order as `tensors`); returns dx or None."""
    lib = _lib.load()
    D = x.shape[1]
    layers, (nw, nb) = _enc_structs(tensors, n_layers)
    glayers, (gnw, gnb) = _enc_structs(grads, n_layers)
    o = _stack_opts(opts)
    dx = torch.empty_like(x) if want_dx else None
    dhidden = dhidden.contiguous()
    rc = lib.sumk_tf_encoder_backward(_p(x), D, dff, n_heads, n_layers, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.cast(layers, C.c_void_p),
                                      _p(nw), _p(nb), C.cast(C.pointer(o), C.c_void_p), _p(dhidden), C.cast(glayers, C.c_void_p),
                                      _p(gnw), _p(gnb), _p(dx), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "sumk_tf_encoder_backward")
    return dx


def _dec_structs(tensors, n_layers):
    nf = len(_lib.TF_DEC_LAYER_FIELDS)
    layers = (_lib.TfDecLayerWeights * n_layers)()
    for l in range(n_layers):
        for i, f in enumerate(_lib.TF_DEC_LAYER_FIELDS):
            setattr(layers[l], f, _ptr(tensors[l * nf + i], f"decoder layer {l} {f}"))
    return layers


def tf_decoder_forward(tgt, memory, sb, tensors, n_layers, n_heads, dff, opts, training=False):
    """Decoder stack (sumk_tf_decoder_forward): tgt, memory (n_rows, D) packed alike -> (out (n_rows, D), workspace).  `tensors`
    in tf_decoder_param_names order."""
    lib = _lib.load()
    _check_rows(tgt, sb, "decoder-stack tgt")
    _check_rows(memory, sb, "decoder-stack memory")
    D = tgt.shape[1]
    layers = _dec_structs(tensors, n_layers)
    o = _stack_opts(opts)
    nbytes = _nonzero(lib.sumk_tf_decoder_workspace_bytes(D, dff, n_heads, n_layers, sb.n_seq, sb.off_host_p), "sumk_tf_decoder_workspace_bytes")
    ws = workspace(nbytes, tgt.device, persistent=training)
    out = torch.empty_like(tgt)
    rc = lib.sumk_tf_decoder_forward(_p(tgt), _p(memory), D, dff, n_heads, n_layers, sb.n_seq, sb.off_host_p, sb.off_dev_p,
                                     C.cast(layers, C.c_void_p), C.cast(C.pointer(o), C.c_void_p), _p(out), _p(ws), ws.numel(),
                                     int(training), _stream())
    _lib.check(rc, "sumk_tf_decoder_forward")
    return out, (ws if training else None)


def tf_decoder_backward(tgt, memory, sb, tensors, grads, n_layers, n_heads, dff, opts, dout, ws, want_dtgt=True, want_dmemory=True):
    """Accumulates into `grads`; returns (dtgt or None, dmemory or None), dmemory summed over the layers."""
    lib = _lib.load()
    D = tgt.shape[1]
    layers = _dec_structs(tensors, n_layers)
    glayers = _dec_structs(grads, n_layers)
    o = _stack_opts(opts)
    dtgt = torch.empty_like(tgt) if want_dtgt else None
    dmem = torch.empty_like(memory) if want_dmemory else None
    dout = dout.contiguous()
    rc = lib.sumk_tf_decoder_backward(_p(tgt), _p(memory), D, dff, n_heads, n_layers, sb.n_seq, sb.off_host_p, sb.off_dev_p,
                                      C.cast(layers, C.c_void_p), C.cast(C.pointer(o), C.c_void_p), _p(dout), C.cast(glayers, C.c_void_p),
                                      _p(dtgt), _p(dmem), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "sumk_tf_decoder_backward")
    return dtgt, dmem


def row_scale_forward(x, s):
    """y[r, :] = x[r, :] * s[r] for x (n_rows, D), s (n_rows,)."""
    lib = _lib.load()
    _require_gpu(x, "row_scale x"); _require_gpu(s, "row_scale s")
    x, s = x.contiguous(), s.contiguous()
    y = torch.empty_like(x)
    _lib.check(lib.sumk_row_scale_forward(_p(x), _p(s), x.shape[0], x.shape[1], _p(y), _stream()), "sumk_row_scale_forward")
    return y


def row_scale_backward(x, s, g, want_dx=True, want_ds=True):
    lib = _lib.load()
    g = g.contiguous()
    dx = torch.empty_like(x) if want_dx else None
    ds = torch.empty_like(s) if want_ds else None
    _lib.check(lib.sumk_row_scale_backward(_p(x), _p(s), _p(g), x.shape[0], x.shape[1], _p(dx), _p(ds), _stream()),
               "sumk_row_scale_backward")
    return dx, ds


# ------------------------------------------------------------------------------------------------ unidirectional LSTM layer / dense layer
def _lstm_dir_struct(cls, tensors):
    s = cls()
    for f, t in zip(("w_ih", "w_hh", "b_ih", "b_hh"), tensors):
        setattr(s, f, _ptr(t, f"LSTM {f}"))
    return s


def _state(t, n_seq, H, what):
    if t is None:
        return None
    _require_gpu(t, what)
    if tuple(t.shape) != (n_seq, H) or not t.is_contiguous():
        raise SumkError(f"{what} must be contiguous ({n_seq}, {H}), got {tuple(t.shape)}")
    return t


def lstm_layer_forward(x, sb, weights, H, h0=None, c0=None, training=False, precision=None):
    """One forward-running LSTM layer (nn.LSTM(bidirectional=False) semantics) on a packed batch.
    x (n_rows, In); weights = (w_ih (4H,In), w_hh (4H,H), b_ih, b_hh); h0 / c0 (n_seq, H) or None.
    Returns (h_out (n_rows, H), h_last (n_seq, H), c_last (n_seq, H), workspace or None)."""
    lib = _lib.load()
    _check_rows(x, sb, "lstm input", col="In")
    In = x.shape[1]
    w = _lstm_dir_struct(_lib.LstmDirWeights, weights)
    h0, c0 = _state(h0, sb.n_seq, H, "h0"), _state(c0, sb.n_seq, H, "c0")
    nbytes = _nonzero(lib.sumk_lstm_workspace_bytes(In, H, sb.n_seq, sb.off_host_p, int(training)), "sumk_lstm_workspace_bytes")
    ws = workspace(nbytes, x.device, persistent=training)
    h = torch.empty(sb.n_rows, H, dtype=torch.float32, device=x.device)
    h_last = torch.empty(sb.n_seq, H, dtype=torch.float32, device=x.device)
    c_last = torch.empty(sb.n_seq, H, dtype=torch.float32, device=x.device)
    rc = lib.sumk_lstm_layer_forward(_p(x), In, H, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(w), _p(h0), _p(c0), _p(h),
                                     _p(h_last), _p(c_last), _p(ws), ws.numel(), int(training), precision_code(precision), _stream())
    _lib.check(rc, "sumk_lstm_layer_forward")
    return h, h_last, c_last, (ws if training else None)


def lstm_layer_backward(x, h, dh, dh_last, dc_last, sb, weights, c0, grads, H, ws, want_dx, want_d0, precision=None):
    """BPTT of one forward-running layer; ACCUMULATES into grads = (dw_ih, dw_hh, db_ih, db_hh).  dh (n_rows, H), dh_last,
    dc_last (n_seq, H) may be None.  Returns (dx or None, dh0 or None, dc0 or None)."""
    lib = _lib.load()
    In = x.shape[1]
    w = _lstm_dir_struct(_lib.LstmDirWeights, weights)
    g = _lstm_dir_struct(_lib.LstmDirGrads, grads)
    dx = torch.empty_like(x) if want_dx else None
    dh0 = torch.empty(sb.n_seq, H, dtype=torch.float32, device=x.device) if want_d0 else None
    dc0 = torch.empty(sb.n_seq, H, dtype=torch.float32, device=x.device) if want_d0 else None
    dh = dh.contiguous() if dh is not None else None
    dh_last = dh_last.contiguous() if dh_last is not None else None
    dc_last = dc_last.contiguous() if dc_last is not None else None
    rc = lib.sumk_lstm_layer_backward(_p(x), _p(h), _p(dh), _p(dh_last), _p(dc_last), In, H, sb.n_seq, sb.off_host_p, sb.off_dev_p,
                                      C.byref(w), _p(c0), C.byref(g), _p(dx), _p(dh0), _p(dc0), _p(ws), ws.numel(),
                                      precision_code(precision), _stream())
    _lib.check(rc, "sumk_lstm_layer_backward")
    return dx, dh0, dc0


def _linear_ws(N, K, device):
    nb = _lib.load().sumk_linear_workspace_bytes(N, K)
    return torch.empty(nb, dtype=torch.uint8, device=device)


def linear_forward(x, w, b, precision=None):
    """y (M, N) = x (M, K) w^T + b, w (N, K) as in nn.Linear."""
    lib = _lib.load()
    _require_gpu(x, "linear input")
    x = x.contiguous()
    M, K = x.shape
    N = w.shape[0]
    ws = _linear_ws(N, K, x.device)
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    _lib.check(lib.sumk_linear_forward(_p(x), _p(w), _p(b), _p(y), M, N, K, _p(ws), ws.numel(), precision_code(precision), _stream()),
               "sumk_linear_forward")
    return y


def linear_backward(x, w, dy, dw, db, want_dx, precision=None):
    """dw (N, K) / db (N) ACCUMULATED if given; returns dx (M, K) or None."""
    lib = _lib.load()
    x, dy = x.contiguous(), dy.contiguous()
    M, K = x.shape
    N = w.shape[0]
    ws = _linear_ws(N, K, x.device)
    dx = torch.empty_like(x) if want_dx else None
    _lib.check(lib.sumk_linear_backward(_p(x), _p(w), _p(dy), M, N, K, _p(dx), _p(dw), _p(db), _p(ws), ws.numel(),
                                        precision_code(precision), _stream()), "sumk_linear_backward")
    return dx


def _dir_array(cls, per_layer):
    arr = (cls * len(per_layer))()
    for l, tensors in enumerate(per_layer):
        for f, t in zip(("w_ih", "w_hh", "b_ih", "b_hh"), tensors):
            setattr(arr[l], f, _ptr(t, f"decoder LSTM {f} (layer {l})"))
    return arr


def lstm_decoder_forward(sb, layers, H, h0=None, c0=None):
    """Step-wise autoregressive decoder (SumGAN's dLSTM): layers = [(w_ih (4H,H), w_hh, b_ih, b_hh)] * L; h0 / c0 (L, n_seq, H)
    or None.  Returns (top-layer outputs (n_rows, H) in time order, workspace)."""
    lib = _lib.load()
    L = len(layers)
    dev = layers[0][0].device
    w = _dir_array(_lib.LstmDirWeights, layers)
    for name, t in (("h0", h0), ("c0", c0)):
        if t is not None:
            _require_gpu(t, f"decoder {name}")
            if tuple(t.shape) != (L, sb.n_seq, H) or not t.is_contiguous():
                raise SumkError(f"decoder {name} must be contiguous ({L}, {sb.n_seq}, {H}), got {tuple(t.shape)}")
    nbytes = _nonzero(lib.sumk_lstm_decoder_workspace_bytes(H, L, sb.n_seq, sb.off_host_p), "sumk_lstm_decoder_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(sb.n_rows, H, dtype=torch.float32, device=dev)
    _lib.check(lib.sumk_lstm_decoder_forward(H, L, sb.n_seq, sb.off_host_p, sb.off_dev_p, w, _p(h0), _p(c0), _p(out), _p(ws), nbytes,
                                             _stream()), "sumk_lstm_decoder_forward")
    return out, ws


def lstm_decoder_backward(sb, layers, H, c0, out, dout, grads, ws, want_d0):
    """grads = [(dw_ih, dw_hh, db_ih, db_hh)] * L, ACCUMULATED.  Returns (dh0, dc0) (L, n_seq, H) or (None, None)."""
    lib = _lib.load()
    L = len(layers)
    w = _dir_array(_lib.LstmDirWeights, layers)
    g = _dir_array(_lib.LstmDirGrads, grads)
    dh0 = torch.empty(L, sb.n_seq, H, dtype=torch.float32, device=out.device) if want_d0 else None
    dc0 = torch.empty(L, sb.n_seq, H, dtype=torch.float32, device=out.device) if want_d0 else None
    _lib.check(lib.sumk_lstm_decoder_backward(H, L, sb.n_seq, sb.off_host_p, sb.off_dev_p, w, _p(c0), _p(out), _p(dout.contiguous()), g,
                                              _p(dh0), _p(dc0), _p(ws), ws.numel(), _stream()), "sumk_lstm_decoder_backward")
    return dh0, dc0


# ------------------------------------------------------------------------------------------------ GRU cell (DSN(cell="gru"))
def gru_cell_forward(gx, gh, h_prev, mask, save=True):
    """One fused GRU step for B sequences: gx, gh (B, 3H), h_prev (B, H), mask (B,) or None -> (h (B, H), rzn (B, 3H) or None)."""
    lib = _lib.load()
    _require_gpu(gx, "gru_cell gx")
    B, H = h_prev.shape
    h = torch.empty_like(h_prev)
    rzn = torch.empty_like(gx) if save else None
    _lib.check(lib.sumk_gru_cell_forward(_p(gx), _p(gh), _p(h_prev), _p(mask), _p(h), _p(rzn), B, H, _stream()), "sumk_gru_cell_forward")
    return h, rzn


def gru_cell_backward(dh, rzn, gh, h_prev, mask):
    """-> (dgx (B, 3H), dgh (B, 3H), direct part of dh_prev (B, H))."""
    lib = _lib.load()
    B, H = h_prev.shape
    dgx, dgh, dhp = torch.empty_like(gh), torch.empty_like(gh), torch.empty_like(h_prev)
    _lib.check(lib.sumk_gru_cell_backward(_p(dh.contiguous()), _p(rzn), _p(gh), _p(h_prev), _p(mask), _p(dgx), _p(dgh), _p(dhp), B, H,
                                          _stream()), "sumk_gru_cell_backward")
    return dgx, dgh, dhp


# ------------------------------------------------------------------------------------------------ BiGRU layer (persistent recurrence, H <= 256)
BIGRU_MAX_H = 256


def bigru_eligible(In, H):
    """The domain of the persistent GRU layer (csrc/gru_persist.hip) on a device whose persistent kernels are usable; other shapes run
    the step path (gru_cell_forward / gru_cell_backward under the host loop of models/_bilstm.py)."""
    return 0 < H <= BIGRU_MAX_H and H % 4 == 0 and In > 0 and In % 4 == 0 and _persistent_ok()


_PERSIST_OK = {}


def _persistent_ok():
    """What csrc/lstm.hip's persistent_kernels_usable() answers: the full chip (256 CUs) and SUMK_LSTM_PERSIST != 0."""
    dev = torch.cuda.current_device()
    ok = _PERSIST_OK.get(dev)
    if ok is None:
        ok = _PERSIST_OK[dev] = (torch.cuda.get_device_properties(dev).multi_processor_count >= 256 and
                                 os.environ.get("SUMK_LSTM_PERSIST", "1")[:1] != "0")
    return ok


def _gru_structs(weights, grads=None):
    """weights / grads: (w_ih, w_hh, b_ih, b_hh) of the forward direction, then of the reverse one."""
    w = _lib.GruLayerWeights()
    g = _lib.GruLayerGrads() if grads is not None else None
    for d in range(2):
        for i, f in enumerate(("w_ih", "w_hh", "b_ih", "b_hh")):
            getattr(w, f)[d] = _ptr(weights[4 * d + i], f"GRU {f} (direction {d})")
            if g is not None:
                getattr(g, f)[d] = grads[4 * d + i].data_ptr()
    return w, g


def bigru_workspace_bytes(In, H, sb, training):
    return _nonzero(_lib.load().sumk_bigru_workspace_bytes(int(In), int(H), sb.n_seq, sb.off_host_p, int(training)), "sumk_bigru_workspace_bytes")


def bigru_layer_forward(x, sb, weights, H, training=False, precision=None, ws=None):
    """x: (n_rows, In) packed -> h (n_rows, 2H) = [h_fwd || h_rev] of one bidirectional nn.GRU layer.  Returns (h, workspace or None).
    ws: a caller-owned workspace (tests); otherwise inference shares the per-stream scratch and a training forward gets its own."""
    lib = _lib.load()
    _check_rows(x, sb, "bigru input", col="In")
    In = x.shape[1]
    w, _ = _gru_structs(weights)
    if ws is None:
        ws = workspace(bigru_workspace_bytes(In, H, sb, training), x.device, persistent=training)
    h = torch.empty(sb.n_rows, 2 * H, dtype=torch.float32, device=x.device)
    rc = lib.sumk_bigru_layer_forward(_p(x), In, H, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(w), _p(h), _p(ws), ws.numel(),
                                      int(training), precision_code(precision), _stream())
    _lib.check(rc, "sumk_bigru_layer_forward")
    if CHECK_LSTM:
        _lib.check(lib.sumk_bigru_check(_p(ws), In, H, sb.n_seq, sb.off_host_p, int(training), 0, _stream()), "sumk_bigru_check")
    return h, (ws if training else None)


def bigru_layer_backward(x, h, dh, sb, weights, grads, H, ws, want_dx, precision=None):
    """BPTT of one bidirectional GRU layer; ACCUMULATES into grads (same order as weights).  Returns dx (n_rows, In) or None."""
    lib = _lib.load()
    In = x.shape[1]
    w, g = _gru_structs(weights, grads)
    dx = torch.empty_like(x) if want_dx else None
    if not dh.is_contiguous():
        dh = dh.contiguous()
    rc = lib.sumk_bigru_layer_backward(_p(x), _p(h), _p(dh), In, H, sb.n_seq, sb.off_host_p, sb.off_dev_p, C.byref(w), C.byref(g),
                                       _p(dx), _p(ws), ws.numel(), precision_code(precision), _stream())
    _lib.check(rc, "sumk_bigru_layer_backward")
    if CHECK_LSTM:
        _lib.check(lib.sumk_bigru_check(_p(ws), In, H, sb.n_seq, sb.off_host_p, 1, 1, _stream()), "sumk_bigru_check")
    return dx
