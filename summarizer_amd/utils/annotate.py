"""Trainable dataset records from raw annotations, on the device.

`Trainer`, `Trainer.test` and `predict_dataset` read records that already hold `gtscore`, `gtsummary`, `user_scores`, `user_summary`,
`change_points`, `n_frame_per_seg` and `picks`; the reference's files were prepared offline by other projects' code
(summarizer/datasets/README.md:50-74).  This module is that preparation for anyone's own annotated videos:

  protocol "scores"     TVSum style -- annotators grade every frame in [lo, hi].  user_scores = the grades rescaled to [0, 1]; gtscore = the
                        annotators' mean at the picks, min-max normalised; user_summary = each annotator's own key-shot summary (KTS
                        segments + a knapsack under `proportion` of the frames, on the annotator's frame-level scores).
  protocol "summaries"  SumMe style -- annotators mark frames (any value > 0).  user_summary = the marks as 0 / 1; gtscore = the fraction
                        of annotators who marked the frame, at the picks; user_scores = that one row upsampled to the frames.
  both                  gtsummary = the key-shot summary of gtscore, sampled at the picks.

`annotate_batch` is the device chain: `sumk_annotate` (csrc/annotate.hip), `sumk_eval_device_segments`, ONE `sumk_eval_device_select` call
with a knapsack / rank problem per annotator row, `sumk_annotate_gtsummary` -- four enqueued calls, no torch arithmetic, nothing copied
home, no host synchronisation.  `build_records` wraps it from numpy in to a `DictDataset` out, with `sumk_kts` + `sumk_kts_segments` in
front for videos that come without change points; `python -m summarizer_amd.utils.annotate IN.npz OUT.npz` is the same from a file.
The specification is tests/annotate_ref.py; the device results equal it bit for bit."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .. import kernels
from .._lib import SumkError
from . import eval_native
from . import kts
from .datasets import DictDataset
from .eval_native import SelectStatusError

PROTOCOLS = {"scores": 0, "summaries": 1}
MAX_USERS, MAX_PICKS, MAX_SEGS, MAX_FRAMES = eval_native.SELECT_MAX_USERS, 4095, eval_native.SELECT_MAX_SEGS, eval_native.SELECT_MAX_FRAMES
_ALIGN = 256


def _protocol(protocol):
    if protocol not in PROTOCOLS:
        raise KeyError(f"Unknown protocol {protocol}")
    return PROTOCOLS[protocol]


def _method(method):
    if method not in eval_native.METHODS:
        raise KeyError(f"Unknown method {method}")
    return eval_native.METHODS[method]


def _score_range(score_range, code):
    lo, hi = float(score_range[0]), float(score_range[1])
    if code == 0 and not (np.isfinite(lo) and np.isfinite(hi) and np.float32(hi) > np.float32(lo)):
        raise SumkError(f"annotate: score_range {tuple(score_range)} must be finite with hi > lo (in float32)")
    return lo, hi


def refusal(n_users, n_frames, n_picks, n_segs, proportion):
    """None when a video of this geometry is within the limits of the chain (sumk_annotate and the kernels behind it), else the limit it is
    past, in words."""
    if not 1 <= n_users <= MAX_USERS:
        return f"{n_users} annotators (1 .. {MAX_USERS})"
    if not 1 <= n_picks <= MAX_PICKS:
        return f"{n_picks} picks (1 .. {MAX_PICKS})"
    return eval_native.select_refusal(n_segs, n_frames, 0, proportion)


class AnnotateChain:
    """The buffers and descriptors of one `annotate_batch` call, built once; `enqueue()` is the four calls on the current stream and
    nothing else (fixed buffers: it can be captured into a HIP graph and replayed).

    annos[v] (U_v, n_frames_v) float32, picks[v] (n_picks_v,) int32: contiguous device tensors.  segments[v]: (change_points (S_v, 2),
    n_frame_per_seg (S_v,)) contiguous int32 device tensors -- or None for the videos of `pending`.
    pending = (P, count): `count` videos (those whose segments[v] is None, in order) get their segments later, at a fixed pitch of P per
    video: the chain owns `pending_cps` (count, P, 2), `pending_nfps` (count, P) and `pending_n_cps` (count,) for `sumk_kts_segments` to fill
    before `enqueue()`.
    summary_lens: per video, sum(n_frame_per_seg) where the caller has a host copy (None, or None entries: the caller vouches that the
    segments tile the frames, as the padded segments of `sumk_kts_segments` do); `sumk_annotate` refuses a video whose sum is not n_frames.
    _gap (tests only): elements left unused behind every video's range in every output -- they must stay as they were.
    Every output lives in ONE allocation (`arena`, bytes): `to_host()` is a single D2H."""

    def __init__(self, annos, picks, n_frames, segments, protocol="scores", score_range=(1, 5), proportion=0.15, method="knapsack",
                 pending=None, summary_lens=None, _gap=0):
        self.protocol, self.method = _protocol(protocol), _method(method)
        self.lo, self.hi = _score_range(score_range, self.protocol)
        n = self.n = len(annos)
        if n == 0:
            raise SumkError("annotate: no videos")
        if not (len(picks) == len(n_frames) == len(segments) == n):
            raise SumkError("annotate: annos, picks, n_frames and segments must have one entry per video")
        dev = self.device = annos[0].device
        P, n_pending = (int(pending[0]), int(pending[1])) if pending else (0, 0)
        if sum(s is None for s in segments) != n_pending:
            raise SumkError("annotate: `pending` must count the videos that come without segments")
        self.nf = nf = [int(f) for f in n_frames]
        self.U, self.NP, self.S = [], [], []
        for v in range(n):
            a, pk = annos[v], picks[v]
            kernels._require_gpu(a, "annotations")
            if not pk.is_cuda:
                raise SumkError(f"annotate: video {v}: picks must be a GPU tensor (no CPU fallback)")
            if a.dtype != torch.float32 or a.dim() != 2 or not a.is_contiguous() or a.shape[1] != nf[v]:
                raise SumkError(f"annotate: video {v}: annotations must be contiguous float32 (n_users, n_frames = {nf[v]}), got {a.dtype} {tuple(a.shape)}")
            if pk.dtype != torch.int32 or pk.dim() != 1 or not pk.is_contiguous():
                raise SumkError(f"annotate: video {v}: picks must be a contiguous int32 vector, got {pk.dtype} {tuple(pk.shape)}")
            if segments[v] is None:
                S = P
            else:
                cp, nfps = segments[v]
                if (cp.dtype != torch.int32 or cp.dim() != 2 or cp.shape[1] != 2 or not cp.is_contiguous() or nfps.dtype != torch.int32
                        or nfps.dim() != 1 or nfps.shape[0] != cp.shape[0] or not nfps.is_contiguous() or not cp.is_cuda or not nfps.is_cuda):
                    raise SumkError(f"annotate: video {v}: segments must be contiguous int32 device tensors (S, 2) and (S,)")
                S = int(cp.shape[0])
            why = refusal(int(a.shape[0]), nf[v], int(pk.shape[0]), S, proportion)
            if why is not None:
                raise SumkError(f"annotate: video {v} has {why}: past the limits of the device chain")
            self.U.append(int(a.shape[0])); self.NP.append(int(pk.shape[0])); self.S.append(S)
        self.cap = [eval_native.select_capacity(f, proportion) for f in nf]
        rows = [u + 1 if self.protocol == 0 else 1 for u in self.U]          # selection problems per video: the annotators' rows + gtscore
        self.n_prob = sum(rows)
        g = int(_gap)
        lens_given = [None] * n if summary_lens is None else list(summary_lens)
        if len(lens_given) != n:
            raise SumkError("annotate: summary_lens must have one entry per video")

        # ---- one allocation for every output; per video and output: (first element, elements)
        def place(counts):
            at, out = 0, []
            for c in counts:
                out.append((at, c)); at += c + g
            return out, at
        self.layout, sizes = {}, {}
        plan = {"user": [u * f for u, f in zip(self.U, nf)], "consensus": nf, "gtscore": self.NP, "gt_seg_means": self.S, "frame_scores": nf,
                "summary": [r * f for r, f in zip(rows, nf)], "gtsummary": self.NP, "selected": [r * s for r, s in zip(rows, self.S)]}
        if self.protocol == 0:
            plan["seg_means"] = [u * s for u, s in zip(self.U, self.S)]
        for name, counts in plan.items():
            self.layout[name], sizes[name] = place(counts)
        if max(sizes.values()) >= 2 ** 31:
            raise SumkError("annotate: the batch is past 2^31 elements in one output (the segments kernel's offsets are int32): split it")
        # status and F-scores (NaN: no annotator masks are given) of the selection problems: one entry per problem, in problem order
        sizes.update(status=self.n_prob, f=2 * self.n_prob)
        dtypes = {"selected": torch.uint8, "status": torch.int32, "f": torch.float64}
        if n_pending:
            sizes.update(pending_cps=n_pending * P * 2, pending_nfps=n_pending * P, pending_n_cps=n_pending)
            dtypes.update(pending_cps=torch.int32, pending_nfps=torch.int32, pending_n_cps=torch.int32)
        at, self._carve = 0, {}
        for name, count in sizes.items():
            dt = dtypes.get(name, torch.float32)
            nbytes = count * torch.empty(0, dtype=dt).element_size()
            self._carve[name] = (at, nbytes, dt)
            at += (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
        self.arena = torch.empty(max(at, _ALIGN), dtype=torch.uint8, device=dev)
        self.buf = {name: self.arena[a:a + nb].view(dt) for name, (a, nb, dt) in self._carve.items()}
        if n_pending:
            self.pending_cps = self.buf["pending_cps"].view(n_pending, P, 2)
            self.pending_nfps = self.buf["pending_nfps"].view(n_pending, P)
            self.pending_n_cps = self.buf["pending_n_cps"]

        # ---- descriptors
        av, ev, sv = (_lib.AnnotateVideo * n)(), (_lib.EvalDevVideo * n)(), (_lib.EvalDevSelect * self.n_prob)()
        L, q, k = self.layout, 0, 0
        self._keep = (annos, picks, segments)
        for v in range(n):
            if segments[v] is None:
                cp_ptr, nfps_ptr = self.pending_cps[k].data_ptr(), self.pending_nfps[k].data_ptr()
                k += 1
            else:
                cp_ptr, nfps_ptr = segments[v][0].data_ptr(), segments[v][1].data_ptr()
            U, S, F = self.U[v], self.S[v], nf[v]
            a = av[v]
            a.anno, a.picks, a.cps = annos[v].data_ptr(), picks[v].data_ptr(), cp_ptr
            a.n_users, a.n_frames, a.n_picks, a.n_segs = U, F, self.NP[v], S
            a.summary_len = F if lens_given[v] is None else int(lens_given[v])
            a.user0, a.frame0, a.pick0 = L["user"][v][0], L["consensus"][v][0], L["gtscore"][v][0]
            a.seg0 = L["seg_means"][v][0] if self.protocol == 0 else 0
            a.gtsum0 = L["summary"][v][0] + (rows[v] - 1) * F                                      # the last row of the video's summary block
            e = ev[v]
            e.picks, e.n_picks, e.n_frames, e.n_steps = picks[v].data_ptr(), self.NP[v], F, self.NP[v]
            e.row0, e.frame0, e.cps, e.n_segs, e.seg0 = L["gtscore"][v][0], L["frame_scores"][v][0], cp_ptr, S, L["gt_seg_means"][v][0]
            for r in range(rows[v]):
                d = sv[q]
                if r < rows[v] - 1:
                    d.seg_means = self.buf["seg_means"].data_ptr() + 4 * (L["seg_means"][v][0] + r * S)
                else:
                    d.seg_means = self.buf["gt_seg_means"].data_ptr() + 4 * L["gt_seg_means"][v][0]
                d.nfps, d.n_segs, d.n_frames, d.capacity, d.summary_len = nfps_ptr, S, F, self.cap[v], F
                d.summary0, d.sel0, d.method = L["summary"][v][0] + r * F, L["selected"][v][0] + r * S, self.method
                q += 1
        self._av, self._ev, self._sv = av, ev, sv
        up = lambda arr: torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)
        self._av_dev, self._ev_dev, self._sv_dev = up(av), up(ev), up(sv)
        lib = _lib.load()
        nb = lib.sumk_eval_device_select_workspace_bytes(self.n_prob, max(self.S), max(self.cap))
        self.ws = kernels.workspace(kernels._nonzero(nb, "sumk_eval_device_select_workspace_bytes"), dev, persistent=True)
        self._sizes = sizes
        self._status, self._f = self.buf["status"], self.buf["f"]

    def enqueue(self):
        """sumk_annotate -> sumk_eval_device_segments -> sumk_eval_device_select -> sumk_annotate_gtsummary on the current stream."""
        lib, b, s = _lib.load(), self.buf, self._sizes
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        seg = b["seg_means"].data_ptr() if self.protocol == 0 else None
        _lib.check(lib.sumk_annotate(self._av_dev.data_ptr(), C.cast(self._av, C.c_void_p), self.n, self.protocol, self.lo, self.hi,
                                     b["user"].data_ptr(), s["user"], b["consensus"].data_ptr(), s["consensus"], b["gtscore"].data_ptr(), s["gtscore"],
                                     seg, s.get("seg_means", 0), st), "sumk_annotate")
        _lib.check(lib.sumk_eval_device_segments(b["gtscore"].data_ptr(), self._ev_dev.data_ptr(), self.n, b["frame_scores"].data_ptr(),
                                                 b["gt_seg_means"].data_ptr(), st), "sumk_eval_device_segments")
        _lib.check(lib.sumk_eval_device_select(self._sv_dev.data_ptr(), C.cast(self._sv, C.c_void_p), self.n_prob, b["summary"].data_ptr(), s["summary"],
                                               b["selected"].data_ptr(), s["selected"], self._f.data_ptr(), self._f.data_ptr() + 8 * self.n_prob,
                                               self._status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), st), "sumk_eval_device_select")
        _lib.check(lib.sumk_annotate_gtsummary(self._av_dev.data_ptr(), C.cast(self._av, C.c_void_p), self.n, b["summary"].data_ptr(), s["summary"],
                                               b["gtsummary"].data_ptr(), s["gtsummary"], st), "sumk_annotate_gtsummary")

    def views(self, buf=None):
        """Per video, the results as views of `buf` (default: the device buffers; `to_host()` for numpy): user_scores, user_summary, gtscore,
        gtsummary -- the record's fields -- and consensus, seg_means (protocol "scores"), gt_seg_means, gt_frame_summary, user_selected
        (protocol "scores"), gt_selected, status (one int32 per selection problem of the video, the gtscore row last)."""
        b, L, out, q = self.buf if buf is None else buf, self.layout, [], 0
        for v in range(self.n):
            U, S, F = self.U[v], self.S[v], self.nf[v]
            rows = U + 1 if self.protocol == 0 else 1
            cut = lambda name: b[name][L[name][v][0]:L[name][v][0] + L[name][v][1]]
            user, summ, sel = cut("user").reshape(U, F), cut("summary").reshape(rows, F), cut("selected").reshape(rows, S)
            d = {"consensus": cut("consensus"), "gtscore": cut("gtscore"), "gtsummary": cut("gtsummary"), "gt_seg_means": cut("gt_seg_means"),
                 "gt_frame_summary": summ[rows - 1], "gt_selected": sel[rows - 1], "status": b["status"][q:q + rows]}
            if self.protocol == 0:
                d.update(user_scores=user, user_summary=summ[:U], user_selected=sel[:U], seg_means=cut("seg_means").reshape(U, S))
            else:
                d.update(user_summary=user, user_scores=cut("frame_scores").reshape(1, F))
            out.append(d)
            q += rows
        return out

    def to_host(self):
        """ONE D2H of the arena (synchronises), then numpy views of it keyed like `buf`."""
        raw = self.arena.cpu().numpy()
        np_dt = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8, torch.float64: np.float64}
        return {name: raw[a:a + nb].view(np_dt[dt]) for name, (a, nb, dt) in self._carve.items()}


def annotate_batch(annos, picks, n_frames, segments, protocol="scores", score_range=(1, 5), proportion=0.15, method="knapsack", summary_lens=None):
    """The device chain for a batch of videos: device tensors in (see `AnnotateChain`), a list of dicts of device tensors out (see
    `AnnotateChain.views`).  Only enqueues work on the current stream.  The picks must ascend inside 0 .. n_frames - 1: the caller's to
    guarantee (they are device memory here; `build_records` checks its host copy).  summary_lens: sum(n_frame_per_seg) per video where the
    caller knows it on the host -- a video whose segments do not tile its frames is then refused before anything is launched; without it
    the caller vouches for the tiling (segments that do not tile surface as a selection status 3 at best)."""
    chain = AnnotateChain(annos, picks, n_frames, segments, protocol, score_range, proportion, method, summary_lens=summary_lens)
    chain.enqueue()
    return chain.views()


def _host_video(key, v):
    """One entry of `videos` as contiguous numpy arrays, with every check the host can make.  Picks ascend, not strictly: equal neighbours
    are allowed, as everywhere in the evaluation tail (the later step owns the frames from there on, eval.py:29-34)."""
    def leaf(name):          # a numpy array, a python value, or an h5py-style leaf
        x = v[name]
        return np.asarray(x) if isinstance(x, (np.ndarray, np.generic, int, float, str, bytes, list, tuple)) else np.asarray(x[...])
    for name in ("features", "picks", "n_frames", "annotations"):
        if name not in v:
            raise SumkError(f"build_records: video {key} has no `{name}`")
    feats = np.ascontiguousarray(leaf("features"), dtype=np.float32)
    picks = np.asarray(leaf("picks"))
    anno = np.ascontiguousarray(leaf("annotations"), dtype=np.float32)
    n_frames = int(np.asarray(leaf("n_frames")).reshape(-1)[0])
    if feats.ndim != 2 or feats.shape[0] < 1:
        raise SumkError(f"build_records: video {key}: features must be (n_steps, D), got {feats.shape}")
    if picks.ndim != 1 or picks.shape[0] != feats.shape[0] or not np.issubdtype(picks.dtype, np.integer):
        raise SumkError(f"build_records: video {key}: picks must be {feats.shape[0]} integers (one per step), got {picks.dtype} {picks.shape}")
    if anno.ndim != 2 or anno.shape[1] != n_frames:
        raise SumkError(f"build_records: video {key}: annotations must be (n_users, n_frames = {n_frames}), got {anno.shape}")
    if not np.all(np.isfinite(anno)):
        raise SumkError(f"build_records: video {key}: annotations must be finite")
    if n_frames < 1 or np.any(np.diff(picks) < 0) or picks[0] < 0 or picks[-1] > n_frames - 1:
        raise SumkError(f"build_records: video {key}: picks must ascend inside 0 .. n_frames - 1 = {n_frames - 1}")
    out = {"features": feats, "picks": np.ascontiguousarray(picks, dtype=np.int32), "annotations": anno, "n_frames": n_frames}
    has_cp, has_nfps = "change_points" in v, "n_frame_per_seg" in v
    if has_cp != has_nfps:
        raise SumkError(f"build_records: video {key}: change_points and n_frame_per_seg come together or not at all")
    if has_cp:
        cp = np.ascontiguousarray(np.asarray(leaf("change_points"))[:, :2], dtype=np.int32)
        nfps = np.ascontiguousarray(leaf("n_frame_per_seg"), dtype=np.int32).reshape(-1)
        if cp.ndim != 2 or cp.shape[0] != nfps.shape[0] or cp.shape[0] < 1:
            raise SumkError(f"build_records: video {key}: change_points {cp.shape} and n_frame_per_seg {nfps.shape} do not match")
        if np.any(nfps < 0) or int(nfps.sum(dtype=np.int64)) != n_frames or np.any(cp[:, 1] - cp[:, 0] + 1 != nfps):
            raise SumkError(f"build_records: video {key}: the segments must tile the video's {n_frames} frames (n_frame_per_seg sums to "
                            f"{int(nfps.sum(dtype=np.int64))})")
        out["change_points"], out["n_frame_per_seg"] = cp, nfps
    if "video_name" in v:
        out["video_name"] = np.asarray(leaf("video_name"))
    return out


def build_records(videos, protocol="scores", score_range=(1, 5), proportion=0.15, method="knapsack", **kts_options):
    """videos: {key: {features (n_steps, D), picks (n_steps,), n_frames, annotations (n_users, n_frames)[, change_points (S, 2),
    n_frame_per_seg (S,), video_name]}} -> a `DictDataset` whose records hold every field of the reference schema (features, picks, n_frames,
    n_steps, change_points, n_frame_per_seg, user_scores, user_summary, gtscore, gtsummary[, video_name]): a trainer opens it unchanged.
    Videos without change points get them from KTS on their features in the same call (kts_options: max_ncp, vmax, lmin, lmax of
    `utils.kts.segment`).  One device chain for the whole set and one D2H at its end.
    Picks ascend inside the video but need not be strictly increasing: of steps that share a frame the last one owns the frames from there
    on (`upsample`), and two KTS change points that fall on one frame leave an EMPTY segment `[f, f - 1]` with `n_frame_per_seg` 0 between
    them in the record (mean 0, never selected, no frames) -- what `utils.kts.cps_to_segments` gives for such picks.
    Raises SumkError for what the host can see before anything is enqueued (shapes, picks that do not ascend inside the video, the limits of
    the chain, a frame budget past SUMK_SELECT_MAX_CAPACITY) and SelectStatusError, naming the video and the row, for what only the
    device sees."""
    code = _protocol(protocol)
    _method(method)
    _score_range(score_range, code)
    unknown = sorted(set(kts_options) - {"max_ncp", "vmax", "lmin", "lmax"})
    if unknown:
        raise TypeError(f"build_records: unknown KTS options {unknown}")
    keys = list(videos.keys())
    if not keys:
        return DictDataset({})
    host = [_host_video(k, videos[k]) for k in keys]
    todo = [i for i, h in enumerate(host) if "change_points" not in h]
    P = 0
    if todo:
        lens = [host[i]["features"].shape[0] for i in todo]
        D = {host[i]["features"].shape[1] for i in todo}
        if len(D) != 1:
            raise SumkError(f"build_records: the videos that need change points must share one feature size, got {sorted(D)}")
        max_ncp = kts_options.get("max_ncp")
        P = min(kts.default_max_ncp(max(lens)) if max_ncp is None else int(max_ncp), max(lens) - 1) + 1
    for k, h in zip(keys, host):
        S = h["change_points"].shape[0] if "change_points" in h else P
        why = refusal(h["annotations"].shape[0], h["n_frames"], h["picks"].shape[0], S, proportion)
        if why is not None:
            raise SumkError(f"build_records: video {k} has {why}: past the limits of the device chain")
    if not torch.cuda.is_available():
        raise SumkError("build_records: no GPU -- summarizer_amd runs only on the HIP path (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(a).to(dev)
    annos, picks = [up(h["annotations"]) for h in host], [up(h["picks"]) for h in host]
    segments = [(up(h["change_points"]), up(h["n_frame_per_seg"])) if "change_points" in h else None for h in host]
    chain = AnnotateChain(annos, picks, [h["n_frames"] for h in host], segments, protocol, score_range, proportion, method,
                          pending=(P, len(todo)) if todo else None,
                          summary_lens=[int(h["n_frame_per_seg"].sum(dtype=np.int64)) if "change_points" in h else None for h in host])
    if todo:
        packed = up(np.concatenate([host[i]["features"] for i in todo]))
        n_cps, cps = kts.segment_packed(packed, lens, **kts_options)
        if int(cps.shape[1]) + 1 != P:
            raise SumkError(f"build_records: KTS returned {int(cps.shape[1]) + 1} segments per video, expected {P}")
        sb = kernels.SeqBatch.get(lens, dev)
        ptrs = up(np.array([picks[i].data_ptr() for i in todo], dtype=np.int64))
        nf_dev = up(np.array([host[i]["n_frames"] for i in todo], dtype=np.int32))
        _lib.check(_lib.load().sumk_kts_segments(n_cps.data_ptr(), cps.data_ptr() if cps.numel() else None, sb.n_seq, P - 1, sb.off_dev_p,
                                                 ptrs.data_ptr(), nf_dev.data_ptr(), chain.pending_cps.data_ptr(), chain.pending_nfps.data_ptr(),
                                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "sumk_kts_segments")
        chain.pending_n_cps.copy_(n_cps)                         # (a device-to-device copy: everything leaves in the one D2H below)
    chain.enqueue()
    raw = chain.to_host()
    kernels.health_check()
    res = chain.views(raw)
    out, k = {}, 0
    for i, (key, h) in enumerate(zip(keys, host)):
        r = res[i]
        bad = np.flatnonzero(r["status"])
        if bad.size:
            row = int(bad[0])
            what = "gtscore" if row == r["status"].shape[0] - 1 else f"annotator {row}"
            raise SelectStatusError(f"build_records: video {key}, row {row} ({what}): sumk_eval_device_select status {int(r['status'][row])} (1: a "
                                    "segment mean is not finite or past 1e12; 2: segment values past the int32 profit rows; 3: bad frames per segment)")
        if "change_points" in h:
            cp, nfps = h["change_points"], h["n_frame_per_seg"]
        else:                                                    # the live segments of the padded layout
            live = int(raw["pending_n_cps"][k]) + 1
            cp = raw["pending_cps"].reshape(-1, P, 2)[k, :live].copy()
            nfps = raw["pending_nfps"].reshape(-1, P)[k, :live].copy()
            k += 1
        rec = {"features": h["features"], "picks": h["picks"], "n_frames": np.int64(h["n_frames"]), "n_steps": np.int64(h["features"].shape[0]),
               "change_points": cp, "n_frame_per_seg": nfps, "user_scores": r["user_scores"].copy(), "user_summary": r["user_summary"].copy(),
               "gtscore": r["gtscore"].copy(), "gtsummary": r["gtsummary"].copy()}
        if "video_name" in h:
            rec["video_name"] = h["video_name"]
        out[key] = rec
    return DictDataset(out)


def main(argv=None):
    """python -m summarizer_amd.utils.annotate IN.npz OUT.npz --protocol scores|summaries [...]: IN holds "<video>/<field>" arrays with the
    fields `build_records` takes; OUT is a dataset file `open_dataset` reads."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m summarizer_amd.utils.annotate", description=main.__doc__)
    ap.add_argument("input"); ap.add_argument("output")
    ap.add_argument("--protocol", choices=sorted(PROTOCOLS), required=True)
    ap.add_argument("--score-range", type=float, nargs=2, default=(1.0, 5.0), metavar=("LO", "HI"))
    ap.add_argument("--proportion", type=float, default=0.15)
    ap.add_argument("--method", choices=sorted(eval_native.METHODS), default="knapsack")
    ap.add_argument("--max-ncp", type=int, default=None); ap.add_argument("--vmax", type=float, default=None)      # KTS, for videos without change points
    ap.add_argument("--lmin", type=int, default=None); ap.add_argument("--lmax", type=int, default=None)
    a = ap.parse_args(argv)
    src = DictDataset.from_npz(a.input)
    videos = {k: {f: leaf[...] for f, leaf in g.items()} for k, g in src.items()}
    opts = {k: v for k, v in (("max_ncp", a.max_ncp), ("vmax", a.vmax), ("lmin", a.lmin), ("lmax", a.lmax)) if v is not None}
    ds = build_records(videos, a.protocol, tuple(a.score_range), a.proportion, a.method, **opts)
    ds.save_npz(a.output)
    print(f"{len(ds)} records -> {a.output}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
