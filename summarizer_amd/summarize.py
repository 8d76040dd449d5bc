"""`Summarizer`: features in, summary out.

The scorers of this package end at per-step importance scores; a key-shot summary also needs the video's change points, which the
reference only ever reads from a prepared dataset file.  `Summarizer` makes them: ONE packed scoring launch (`model.score_packed`) and
ONE change-point call (`sumk_kts`, csrc/kts.hip) on the same packed features, one D2H for both results, then the unchanged key-shot
selection of `utils.eval.generate_summary` (knapsack or rank under the frame budget)."""
import numpy as np
import torch

from . import kernels
from ._lib import SumkError
from .utils import eval as ev
from .utils import kts


class Summarizer:
    """Summarizer(model, proportion=0.15, method="knapsack", **kts_options)

    model: any scorer of this package with `score_packed` (VASNet, DSN, sLSTM, Transformer, ...), on the GPU.
    proportion / method: the summary budget and the selection algorithm of `generate_summary` ("knapsack" | "rank").
    kts_options: max_ncp, vmax, lmin, lmax of `utils.kts.segment` (max_ncp=None: min(n - 1, 1023))."""

    def __init__(self, model, proportion=0.15, method="knapsack", **kts_options):
        if not hasattr(model, "score_packed"):
            raise SumkError(f"Summarizer: {type(model).__name__} has no score_packed")
        unknown = sorted(set(kts_options) - {"max_ncp", "vmax", "lmin", "lmax"})
        if unknown:
            raise TypeError(f"Summarizer: unknown KTS options {unknown}")
        if method not in ("knapsack", "rank"):
            raise KeyError(f"Unknown method {method}")
        self.model, self.proportion, self.method, self.kts_options = model, proportion, method, kts_options

    def summarize(self, features, picks=None, n_frames=None):
        """One video: features (T, D) -> {"scores" (T,) float32, "change_points" (S, 2) int32, "n_frame_per_seg" (S,) int32,
        "machine_summary" (n_frames,) float32 of 0 / 1}.  picks=None: arange(T); n_frames=None: T."""
        return self.summarize_batch([features], [picks], [n_frames])[0]

    def summarize_batch(self, list_of_features, picks=None, n_frames=None):
        """The same for several videos in one scoring launch and one change-point call; picks / n_frames: lists (or None)."""
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
        packed = (feats[0] if len(feats) == 1 else torch.cat(feats)).contiguous()
        was_training = getattr(self.model, "training", False)
        if was_training:
            self.model.eval()
        try:
            with torch.no_grad():
                scores = self.model.score_packed(packed, lens).detach().reshape(-1)
                n_cps, cps = kts.segment_packed(packed, lens, **self.kts_options)
        finally:
            if was_training:
                self.model.train()
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
