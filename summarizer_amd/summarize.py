"""`Summarizer`: features in, summary out.

The scorers of this package end at per-step importance scores; a key-shot summary also needs the video's change points, which the
reference only ever reads from a prepared dataset file.  `Summarizer` makes them: ONE packed scoring launch (`model.score_packed`) and
ONE change-point call (`sumk_kts`, csrc/kts.hip) on the same packed features, one D2H for both results, then the unchanged key-shot
selection of `utils.eval.generate_summary` (knapsack or rank under the frame budget).

`Summarizer(..., device=True)` keeps the whole chain on the device instead: scoring, `sumk_kts`, `sumk_kts_segments` (change points ->
padded segments), `sumk_eval_device_segments` (upsample + segment means) and `sumk_eval_device_select` (key shots + expansion) are
enqueued back to back, nothing is copied home and nothing waits: the results are device tensors.  `tail="long"` puts
`sumk_eval_device_segments_long` and `sumk_eval_device_select_long` (csrc/evallong.hip) in the place of the last two: the same results
without their limits of 4096 steps and a budget of 8191 frames, for the videos `kts="banded"` segments."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import kernels
from ._lib import SumkError
from .utils import eval as ev
from .utils import eval_native
from .utils import kts


class Summarizer:
    """Summarizer(model, proportion=0.15, method="knapsack", device=False, kts="dense", tail="block", max_workspace_bytes=None, **kts_options)

    model: any scorer of this package with `score_packed` (VASNet, DSN, sLSTM, Transformer, ...), on the GPU.
    proportion / method: the summary budget and the selection algorithm of `generate_summary` ("knapsack" | "rank").
    kts_options: max_ncp, vmax, lmin, lmax of `utils.kts.segment` (max_ncp=None: min(n - 1, 1023)).
    kts: "dense" (the default: `sumk_kts`, videos up to 16384 steps) | "banded" (`sumk_kts_banded`: long videos, see `utils.kts.segment_packed`;
    the same change points wherever both apply, and the same output layout, so it goes with device=True as well -- past 4096 steps with
    tail="long").
    device: False (the default) returns numpy arrays after one D2H; True returns device tensors and never synchronises (see
    `summarize_batch`).
    tail (device=True only): "block" (the default: one workgroup per video, at most 4096 steps and a budget of 8191 frames) | "long" (the
    chip-wide kernels: up to 1 048 576 steps, 2^24 frames and any budget; the same results bit for bit).
    max_workspace_bytes: None = `utils.kts.DEFAULT_MAX_WORKSPACE_BYTES`; what the banded KTS and the long tail's selection may ask for."""

    def __init__(self, model, proportion=0.15, method="knapsack", device=False, kts="dense", tail="block", max_workspace_bytes=None, **kts_options):
        if not hasattr(model, "score_packed"):
            raise SumkError(f"Summarizer: {type(model).__name__} has no score_packed")
        unknown = sorted(set(kts_options) - {"max_ncp", "vmax", "lmin", "lmax"})
        if unknown:
            raise TypeError(f"Summarizer: unknown KTS options {unknown}")
        if method not in ("knapsack", "rank"):
            raise KeyError(f"Unknown method {method}")
        if kts not in ("dense", "banded"):
            raise KeyError(f"Unknown kts {kts}")
        if tail not in ("block", "long"):
            raise KeyError(f"Unknown tail {tail}")
        if tail == "long" and not device:
            raise SumkError('Summarizer: tail="long" needs device=True (the host tail has no limits to lift)')
        self.kts, self.tail, self.max_workspace_bytes = kts, tail, max_workspace_bytes
        self.model, self.proportion, self.method, self.kts_options, self.device = model, proportion, method, kts_options, bool(device)

    def summarize(self, features, picks=None, n_frames=None):
        """One video: features (T, D) -> {"scores" (T,) float32, "change_points" (S, 2) int32, "n_frame_per_seg" (S,) int32,
        "machine_summary" (n_frames,) float32 of 0 / 1}.  picks=None: arange(T); n_frames=None: T."""
        return self.summarize_batch([features], [picks], [n_frames])[0]

    def summarize_batch(self, list_of_features, picks=None, n_frames=None):
        """The same for several videos in one scoring launch and one change-point call; picks / n_frames: lists (or None).
        device=True: every value is a device tensor and the call only enqueues work -- "change_points" (P, 2) / "n_frame_per_seg" (P,) are
        padded to P = max_ncp + 1 segments with empty ones behind the live "n_segs" (0-d int32 = change points found + 1), and "status"
        (0-d int32) is sumk_eval_device_select's verdict on the video (0: fine), for the caller to look at when it synchronises anyway."""
        feats = [f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)) for f in list_of_features]
        if not feats:
            return []
        dev = next((p.device for p in self.model.parameters()), None) if hasattr(self.model, "parameters") else None
        if dev is None or dev.type != "cuda":
            dev = next((f.device for f in feats if f.is_cuda), torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
        if dev is None:
            raise SumkError("Summarizer: no GPU -- summarizer_amd runs only on the HIP path (no CPU fallback)")
        feats = [f.reshape(f.shape[0], -1).to(dev, torch.float32) for f in feats]
        lens = [f.shape[0] for f in feats]
        picks = [None] * len(feats) if picks is None else list(picks)
        n_frames = [None] * len(feats) if n_frames is None else list(n_frames)
        if self.device:
            n_frames, picks = (self._check_long_limits if self.tail == "long" else self._check_device_limits)(lens, picks, n_frames)
        packed = (feats[0] if len(feats) == 1 else torch.cat(feats)).contiguous()
        was_training = getattr(self.model, "training", False)
        if was_training:
            self.model.eval()
        try:
            with torch.no_grad():
                scores = self.model.score_packed(packed, lens).detach().reshape(-1)
                n_cps, cps = kts.segment_packed(packed, lens, banded=self.kts == "banded", max_workspace_bytes=self._max_ws(), **self.kts_options)
        finally:
            if was_training:
                self.model.train()
        if self.device:
            return self._finish_on_device(scores.contiguous(), n_cps, cps, lens, picks, n_frames, dev)
        scores = scores.cpu().numpy()
        kernels.health_check()
        segs = kts.segments_from_device(n_cps, cps, lens, picks, n_frames)
        out = []
        for v, (piece, (cp, nfps)) in enumerate(zip(np.split(scores, np.cumsum(lens)[:-1]), segs)):
            pk = np.arange(lens[v], dtype=np.int32) if picks[v] is None else np.asarray(picks[v])
            nf = lens[v] if n_frames[v] is None else int(n_frames[v])
            summary = ev.generate_summary(piece, cp, nf, nfps.tolist(), pk, self.proportion, self.method)
            out.append({"scores": piece.copy(), "change_points": cp, "n_frame_per_seg": nfps, "machine_summary": summary})
        return out

    def _check_device_limits(self, lens, picks, n_frames):
        """device=True, before anything is enqueued: the videos against the limits of the device tail (ascending picks within the video,
        at most 4096 of them) and of sumk_eval_device_select at the padded segment count.  Returns (n_frames per video, picks per video
        as contiguous int32 arrays or None for the identity)."""
        P = self._padded_segments(lens)
        nf = [int(T) if f is None else int(f) for T, f in zip(lens, n_frames)]
        out = []
        for v, (T, pk) in enumerate(zip(lens, picks)):
            if T > 4096:
                raise SumkError(f"Summarizer(device=True): video {v} has {T} picks, the device tail takes 4096")
            why = eval_native.select_refusal(P, nf[v], 0, self.proportion)
            if why is not None:
                raise SumkError(f"Summarizer(device=True): video {v} has {why}: past the limits of sumk_eval_device_select")
            out.append(self._checked_picks(v, T, pk, nf[v]))
        return nf, out

    @staticmethod
    def _checked_picks(v, T, pk, n_frames):
        """The picks of video v as a contiguous int32 array (None: the identity), ascending within 0 .. n_frames as both device tails need."""
        if pk is not None:
            pk = np.ascontiguousarray(np.asarray(pk), dtype=np.int32).reshape(-1)
            if pk.shape[0] != T:
                raise ValueError(f"Summarizer: video {v} has {T} steps but {pk.shape[0]} picks")
            if np.any(np.diff(pk) < 0) or (T and (pk[0] < 0 or pk[-1] > n_frames)):
                raise SumkError(f"Summarizer(device=True): video {v}: picks must ascend within 0 .. n_frames (the device tail's limit)")
        return pk

    def _max_ws(self):
        return kts.DEFAULT_MAX_WORKSPACE_BYTES if self.max_workspace_bytes is None else int(self.max_workspace_bytes)

    def _padded_segments(self, lens):
        max_ncp = self.kts_options.get("max_ncp")
        return min(kts.default_max_ncp(max(lens)) if max_ncp is None else int(max_ncp), max(lens) - 1) + 1

    def _check_long_limits(self, lens, picks, n_frames):
        """device=True, tail="long", before anything is enqueued: the videos against the limits of sumk_eval_device_segments_long (ascending
        picks within the video, at most 1 048 576 of them, at most 2^24 frames) and of sumk_eval_device_select_long at the padded segment
        count, and that call's workspace against max_workspace_bytes.  Returns what _check_device_limits returns."""
        P = self._padded_segments(lens)
        nf = [int(T) if f is None else int(f) for T, f in zip(lens, n_frames)]
        out = []
        for v, (T, pk) in enumerate(zip(lens, picks)):
            if T > eval_native.SEGMENTS_LONG_MAX_PICKS:
                raise SumkError(f'Summarizer(tail="long"): video {v} has {T} picks, the long device tail takes {eval_native.SEGMENTS_LONG_MAX_PICKS}')
            why = eval_native.select_long_refusal(P, nf[v], 0, self.proportion)
            if why is not None:
                raise SumkError(f'Summarizer(tail="long"): video {v} has {why}: past the limits of sumk_eval_device_select_long')
            out.append(self._checked_picks(v, T, pk, nf[v]))
        cap = max(eval_native.select_capacity(f, self.proportion) for f in nf)
        need = eval_native.select_long_workspace_bytes(len(lens), P, cap)
        if need > self._max_ws():
            raise SumkError(f'Summarizer(tail="long"): {len(lens)} videos of {P} padded segments with a budget of {cap} frames need a workspace of {need} '
                            f"bytes, over max_workspace_bytes={self._max_ws()}: use a smaller max_ncp (the workspace grows as segments x budget / 8)")
        return nf, out

    def _finish_on_device(self, scores, n_cps, cps, lens, picks, nf, dev):
        lib, n, P = _lib.load(), len(lens), int(cps.shape[1]) + 1

        def upload(t):      # through pinned memory and asynchronous: a pageable H2D would wait for the scoring and KTS work already enqueued
            return t.pin_memory().to(dev, non_blocking=True)
        identity = torch.arange(max(lens), dtype=torch.int32, device=dev)
        pk_dev = [identity if pk is None else upload(torch.from_numpy(pk)) for pk in picks]
        sb = kernels.SeqBatch.get(lens, dev)
        ptrs = upload(torch.tensor([t.data_ptr() for t in pk_dev], dtype=torch.int64))
        nf_dev = upload(torch.tensor(nf, dtype=torch.int32))
        change_points, nfps = kernels.kts_segments(n_cps, cps, sb, ptrs, nf_dev)
        vd, sd = (_lib.EvalDevVideo * n)(), (_lib.EvalDevSelect * n)()
        seg = torch.empty(n * P, dtype=torch.float32, device=dev)
        frame0 = 0
        for v, T in enumerate(lens):
            e = vd[v]
            e.picks, e.n_picks, e.n_frames, e.n_steps = pk_dev[v].data_ptr(), T, nf[v], T
            e.row0, e.frame0 = int(sb.off_host[v]), frame0
            e.cps, e.n_segs, e.seg0 = change_points[v].data_ptr(), P, v * P
            q = sd[v]
            q.seg_means, q.nfps = seg.data_ptr() + 4 * v * P, nfps[v].data_ptr()
            q.n_segs, q.n_frames, q.capacity = P, nf[v], eval_native.select_capacity(nf[v], self.proportion)
            q.summary_len, q.summary0, q.sel0 = nf[v], frame0, v * P          # (the segments of a video tile its frames: sum(nfps) == n_frames)
            q.method = eval_native.METHODS[self.method]
            frame0 += nf[v]
        vd_dev = upload(torch.frombuffer(bytearray(bytes(vd)), dtype=torch.uint8))
        sd_dev = upload(torch.frombuffer(bytearray(bytes(sd)), dtype=torch.uint8))
        scratch = torch.empty(frame0, dtype=torch.float32, device=dev)
        summary = torch.empty(frame0, dtype=torch.float32, device=dev)
        selected = torch.empty(n * P, dtype=torch.uint8, device=dev)
        f = torch.empty(2 * n, dtype=torch.float64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        if self.tail == "long":
            ws = kernels.workspace(kernels.eval_select_long_workspace_bytes(n, P, max(q.capacity for q in sd)), dev)
            kernels.eval_segments_long(scores, vd_dev, vd, scratch, seg)
            kernels.eval_select_long(sd_dev, sd, summary, selected, f[:n], f[n:], status, ws)
        else:
            ws = kernels.workspace(lib.sumk_eval_device_select_workspace_bytes(n, P, max(q.capacity for q in sd)), dev)
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.sumk_eval_device_segments(scores.data_ptr(), vd_dev.data_ptr(), n, scratch.data_ptr(), seg.data_ptr(), st),
                       "sumk_eval_device_segments")
            _lib.check(lib.sumk_eval_device_select(sd_dev.data_ptr(), C.cast(sd, C.c_void_p), n, summary.data_ptr(), frame0, selected.data_ptr(), n * P,
                                                   f.data_ptr(), f.data_ptr() + 8 * n, status.data_ptr(), ws.data_ptr(), ws.numel(), st),
                       "sumk_eval_device_select")
        out, at = [], 0
        for v, T in enumerate(lens):
            r0 = int(sb.off_host[v])
            out.append({"scores": scores[r0:r0 + T], "change_points": change_points[v], "n_frame_per_seg": nfps[v], "n_segs": n_cps[v] + 1,
                        "machine_summary": summary[at:at + nf[v]], "status": status[v]})
            at += nf[v]
        return out
