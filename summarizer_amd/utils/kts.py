"""Kernel temporal segmentation (KTS, Potapov et al. 2014): change points of a video from its features, on the device
(csrc/kts.hip through kernels.kts*).  The reference has no counterpart -- it reads `change_points` / `n_frame_per_seg` that were
prepared offline with KTS (summarizer/datasets/README.md) -- so this is what turns scores into key shots for any other video.

`cpd_nonlin` / `cpd_auto` keep the names, arguments and return shapes of the original KTS functions; `segment` goes from features to
the `(change_points, n_frame_per_seg)` pair `utils.eval.generate_summary` consumes.  The compute runs in libsumk.so only (no CPU
fallback, as everywhere in this package); `cps_to_segments` is a pure host conversion."""
import numpy as np
import torch

from .. import kernels
from .._lib import SumkError

DEFAULT_MAX_NCP = 1023
DEFAULT_MAX_WORKSPACE_BYTES = 8 << 30      # banded path: refuse, before anything is enqueued, a workspace a shared card should not be asked for


def _gram_on_device(K):
    """(flat float64 device tensor, n) from a square CUDA tensor or numpy array."""
    if isinstance(K, np.ndarray):
        if not torch.cuda.is_available():
            raise SumkError("kts: no GPU -- summarizer_amd runs only on the HIP path (no CPU fallback)")
        K = torch.from_numpy(np.ascontiguousarray(K, dtype=np.float64)).cuda()
    if not torch.is_tensor(K) or not K.is_cuda:
        raise SumkError("kts: K must be a CUDA tensor or a numpy array (no CPU fallback)")
    if K.dim() != 2 or K.shape[0] != K.shape[1] or K.shape[0] < 1:
        raise SumkError(f"kts: K must be a square matrix, got {tuple(K.shape)}")
    return K.to(torch.float64).contiguous().reshape(-1), int(K.shape[0])


def cpd_nonlin(K, ncp, lmin=1, lmax=100000):
    """Change points of the best segmentation of the n steps behind the (n, n) kernel matrix K into exactly ncp + 1 segments.
    Returns (cps (ncp,) int, scores (ncp + 1,) float64): cps ascending, each the first step of a new segment; scores[k] = the optimal
    within-segment scatter with k change points (+inf where no segmentation satisfies lmin / lmax)."""
    flat, n = _gram_on_device(K)
    ncp = int(ncp)
    if not 0 <= ncp <= n - 1:
        raise ValueError(f"cpd_nonlin: ncp={ncp} outside 0 .. n - 1 = {n - 1}")
    sb = kernels.SeqBatch.get([n], flat.device)
    _, cps, scores = kernels.kts_gram_nonlin(flat, sb, ncp, lmin, lmax)
    return cps[0].cpu().numpy().astype(np.int64), scores[0].cpu().numpy()


def cpd_auto(K, ncp, vmax=1.0, lmin=1, lmax=100000):
    """Change points with the number of segments chosen by the KTS penalty: m_best = argmin_k scores[k] / n + (vmax k / (2 n))
    (ln(n / k) + 1) over k = 0 .. ncp (the smallest k at a tie).  Returns (cps (m_best,) int, scores (m_best + 1,) float64)."""
    flat, n = _gram_on_device(K)
    ncp = min(int(ncp), n - 1)
    if ncp < 0:
        raise ValueError(f"cpd_auto: ncp={ncp} is negative")
    sb = kernels.SeqBatch.get([n], flat.device)
    n_cps, cps, scores = kernels.kts_gram(flat, sb, ncp, vmax, lmin, lmax)
    m = int(n_cps[0].item())
    return cps[0, :m].cpu().numpy().astype(np.int64), scores[0, :m + 1].cpu().numpy()


def cps_to_segments(cps, picks, n_frames):
    """Change points in steps -> ((S, 2) int32 change_points in frames, (S,) int32 n_frame_per_seg): the boundaries are the frames
    picks[c]; segments [0, picks[c1] - 1], [picks[c1], picks[c2] - 1], ..., [picks[cm], n_frames - 1] -- the layout
    utils.eval.generate_summary consumes.  Pure host code."""
    cps = np.asarray(cps, dtype=np.int64).reshape(-1)
    picks = np.asarray(picks).astype(np.int64).reshape(-1)
    starts = np.concatenate([[0], picks[cps]])
    ends = np.concatenate([picks[cps] - 1, [int(n_frames) - 1]])
    change_points = np.stack([starts, ends], axis=1).astype(np.int32)
    return change_points, (ends - starts + 1).astype(np.int32)


def cps_to_segments_padded(cps, picks, n_frames, n_segs):
    """cps_to_segments at a fixed number of segments: the live ones first, then EMPTY segments -- change_points (n_frames, n_frames - 1),
    n_frame_per_seg 0 -- up to n_segs.  An empty segment has mean 0, never improves a knapsack capacity and adds no frame in rank mode, so
    utils.eval.generate_summary gives the summary of the unpadded segments.  The specification of sumk_kts_segments (csrc/evalselect.hip),
    which builds this layout on the device so that the segment count of a video stays a host-known bound."""
    change_points, nfps = cps_to_segments(cps, picks, n_frames)
    pad = int(n_segs) - change_points.shape[0]
    if pad < 0:
        raise ValueError(f"cps_to_segments_padded: {change_points.shape[0]} segments do not fit n_segs={n_segs}")
    empty = np.tile(np.array([[int(n_frames), int(n_frames) - 1]], dtype=np.int32), (pad, 1))
    return np.concatenate([change_points, empty]), np.concatenate([nfps, np.zeros(pad, dtype=np.int32)])


def default_max_ncp(n):
    return min(int(n) - 1, DEFAULT_MAX_NCP)


def segment_packed(x, lens, max_ncp=None, vmax=1.0, lmin=1, lmax=100000, banded=False, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """Device half of `segment`: (n_cps, cps) device tensors for a packed batch; only enqueues work.
    banded=True: the long-video path (sumk_kts_banded: up to 1 048 576 steps per video, memory O(n min(lmax, n)), a DP row per launch);
    the same change points as the default wherever both accept the input.  It raises SumkError before anything is enqueued when its
    workspace would pass max_workspace_bytes -- a safety condition for shared cards, not a tuning value."""
    sb = kernels.SeqBatch.get(lens, x.device)
    if max_ncp is None:
        max_ncp = default_max_ncp(max(sb.lens))
    max_ncp = min(int(max_ncp), max(sb.lens) - 1)
    if not banded:
        n_cps, cps, _ = kernels.kts(x, sb, max_ncp, vmax, lmin, lmax, want_scores=False)
        return n_cps, cps
    need = kernels.kts_banded_workspace_bytes(x.shape[-1], sb, max_ncp, lmax)
    if need > int(max_workspace_bytes):
        n = max(sb.lens)
        raise SumkError(f"kts banded: n={n} steps with a band of B=min(lmax, n)={min(int(lmax), n)} need a workspace of {need} bytes, over "
                        f"max_workspace_bytes={int(max_workspace_bytes)}: use a smaller lmax (the workspace grows as n * B)")
    n_cps, cps, _ = kernels.kts_banded(x, sb, max_ncp, vmax, lmin, lmax, want_scores=False)
    return n_cps, cps


def segments_from_device(n_cps, cps, lens, picks=None, n_frames=None):
    """Host half of `segment`: one D2H of the change points, then cps_to_segments per video."""
    n_cps, cps = n_cps.cpu().numpy(), cps.cpu().numpy()
    out = []
    for v, n in enumerate(lens):
        pk = np.arange(n) if picks is None or picks[v] is None else picks[v]
        nf = n if n_frames is None or n_frames[v] is None else n_frames[v]
        if len(pk) != n:
            raise ValueError(f"kts.segment: video {v} has {n} steps but {len(pk)} picks")
        out.append(cps_to_segments(cps[v, :n_cps[v]], pk, nf))
    return out


def segment(features, lens=None, picks=None, n_frames=None, max_ncp=None, vmax=1.0, lmin=1, lmax=100000, banded=False,
            max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """KTS change points of one video or of a packed batch, in frames.

    features: one (T, D) float32 CUDA tensor, or the rows of several videos packed back to back with their `lens`.
    picks / n_frames: positions of the steps in the original video and its frame count (per video: lists when `lens` is given);
    None means picks = arange(n) and n_frames = n.  max_ncp=None means min(n - 1, 1023) change points at most (n = the longest video
    of the call); a video shorter than max_ncp + 1 steps is searched up to n - 1.
    banded / max_workspace_bytes: the long-video path of `segment_packed` (set lmax to the longest segment worth looking for).
    Returns (change_points (S, 2) int32, n_frame_per_seg (S,) int32) -- a list of such pairs when `lens` is given."""
    single = lens is None
    if single:
        lens, picks, n_frames = [features.shape[0]], [picks], [n_frames]
    n_cps, cps = segment_packed(features, lens, max_ncp, vmax, lmin, lmax, banded, max_workspace_bytes)
    out = segments_from_device(n_cps, cps, [int(v) for v in lens], picks, n_frames)
    return out[0] if single else out
