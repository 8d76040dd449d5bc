"""Inter-annotator agreement on the device: the "human" row of the evaluation protocol.

`Trainer.test` reports a model's distance to the annotators -- the mean key-shot F-score against `user_summary` and the mean rank
correlation against `user_scores`.  This module is the other half: how well the annotators agree with EACH OTHER under the same two
metrics, per video and over a set, for anyone who has `user_summary` / `user_scores` (a dataset file, or the records
`utils.annotate.build_records` just made):

  F[a][b]   evaluate_summary(user_summary[a], user_summary[b:b+1]) -- annotator a in the machine's place (eval.py:125-165), float32
  C[a][b]   Spearman's rho or Kendall's tau-b of the two annotators' frame scores (evaluate_scores, eval.py:49-72), float64
  per annotator: the mean (F: and the maximum) over the OTHER annotators -- leave-one-out; per video: the mean of those over the annotators.

`AgreementChain` is the device chain: `sumk_rank_rows` (average ranks, dense ranks, tie counts -- what `eval.rank_users` and
`eval_native._kendall_meta` compute on the host), `sumk_agreement_f`, `sumk_agreement_corr` (csrc/agreement.hip) -- three enqueued calls,
no torch arithmetic, no host synchronisation.  `human_agreement` wraps it: one upload, one enqueue, one D2H.  `python -m
summarizer_amd.utils.agreement DATA.npz` prints the row for a dataset file.  The specification is tests/agreement_ref.py; the device
results equal it bit for bit."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .. import kernels
from .._lib import SumkError
from . import eval as ev
from . import eval_native

METRICS = {"spearmanr": 0, "kendalltau": 1}
MAX_USERS, MAX_FRAMES, MAX_RANK_FRAMES = eval_native.SELECT_MAX_USERS, eval_native.SELECT_MAX_FRAMES, eval_native.KENDALL_MAX_FRAMES
_ALIGN = 256
_NP = {torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64, torch.float64: np.float64}


def _metric(metric):
    if metric not in METRICS:
        raise KeyError(f"Unknown metric {metric}")
    return METRICS[metric]


def refusal(n_sum, n_sc, n_frames):
    """None when a video of this geometry is within the limits of the device chain, else the limit it is past, in words.  (A video past
    MAX_RANK_FRAMES with scores is not refused by `human_agreement`: its correlation takes the host path.)"""
    if not 0 <= n_sum <= MAX_USERS:
        return f"{n_sum} annotators in user_summary (at most {MAX_USERS})"
    if not 0 <= n_sc <= MAX_USERS:
        return f"{n_sc} annotators in user_scores (at most {MAX_USERS})"
    if not 1 <= n_frames <= MAX_FRAMES:
        return f"{n_frames} frames (1 .. {MAX_FRAMES})"
    if n_sc > 0 and n_frames > MAX_RANK_FRAMES:
        return f"{n_frames} frames (ranks and correlations: at most {MAX_RANK_FRAMES})"
    return None


def _check_rows(t, v, what):
    kernels._require_gpu(t, f"agreement: video {v}: {what}")
    if t.dim() != 2 or not t.is_contiguous():
        raise SumkError(f"agreement: video {v}: {what} must be contiguous float32 (n_users, n_frames), got {tuple(t.shape)}")


class AgreementChain:
    """The buffers and descriptors of one batch, built once; `enqueue()` is the three calls on the current stream and nothing else (fixed
    buffers: it can be captured into a HIP graph and replayed).

    summaries[v] / scores[v]: contiguous float32 device tensors (n_users, n_frames_v), or None -- the two may differ in n_users, not in
    n_frames.  A video without scores takes no part in the ranks and correlations, one without summaries none in F; their per-video
    results are NaN.
    _gap (tests only): elements left unused behind every video's range in every buffer -- they must stay as they were.
    _sort_only (tests only): Kendall with every pair through the LDS sort, also where the contingency-table path would take it.
    Results live in ONE allocation (`arena`, bytes): `to_host()` is a single D2H.  The ranks (float64 + int32 per frame and annotator, by
    far the largest buffers) live in a second one, `scratch`, which stays on the device."""

    def __init__(self, summaries, scores, metric="spearmanr", _gap=0, _sort_only=False):
        self.metric = _metric(metric)
        self._code = 2 if (_sort_only and self.metric == 1) else self.metric      # SUMK_AGREEMENT_KENDALL_SORT
        n = self.n = len(summaries)
        if n == 0:
            raise SumkError("agreement: no videos")
        if len(scores) != n:
            raise SumkError("agreement: summaries and scores must have one entry per video")
        if n > 65535:
            raise SumkError(f"agreement: {n} videos (at most 65535 per chain): split the batch")
        self.Us, self.Uc, self.nf = [], [], []
        dev = None
        for v in range(n):
            s, x = summaries[v], scores[v]
            if s is None and x is None:
                raise SumkError(f"agreement: video {v} has neither user_summary nor user_scores")
            for t, what in ((s, "user_summary"), (x, "user_scores")):
                if t is not None:
                    _check_rows(t, v, what)
                    dev = t.device if dev is None else dev
            if s is not None and x is not None and s.shape[1] != x.shape[1]:
                raise SumkError(f"agreement: video {v}: user_summary spans {s.shape[1]} frames, user_scores {x.shape[1]}")
            us, uc = 0 if s is None else int(s.shape[0]), 0 if x is None else int(x.shape[0])
            nf = int((s if s is not None else x).shape[1])
            why = refusal(us, uc, nf)
            if why is not None:
                raise SumkError(f"agreement: video {v} has {why}: past the limits of the device chain")
            self.Us.append(us); self.Uc.append(uc); self.nf.append(nf)
        self.device = dev
        self.has_f, self.has_corr = any(self.Us), any(self.Uc)
        g = int(_gap)

        def place(counts):
            at, out = 0, []
            for c in counts:
                out.append((at, c)); at += c + g
            return out, at
        L, size = {}, {}
        for name, counts in (("rank", [u * f for u, f in zip(self.Uc, self.nf)]), ("row", self.Uc), ("sum", self.Us),
                             ("F", [u * u for u in self.Us]), ("C", [u * u for u in self.Uc])):
            L[name], size[name] = place(counts)
        self.layout, self.size = L, size

        def carve(plan):
            at, out = 0, {}
            for name, (count, dt) in plan.items():
                nbytes = count * torch.empty(0, dtype=dt).element_size()
                out[name] = (at, nbytes, dt)
                at += (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
            return out, max(at, _ALIGN)
        f64, f32, i64, i32 = torch.float64, torch.float32, torch.int64, torch.int32
        plan = {"ties": (size["row"], i64), "mean": (size["row"], f64), "ssq": (size["row"], f64), "corr_user": (size["row"], f64),
                "C": (size["C"], f64), "f_avg": (n, f64), "f_max": (n, f64), "corr": (n, f64), "F": (size["F"], f32),
                "f_avg_user": (size["sum"], f32), "f_max_user": (size["sum"], f32)}
        if self.metric == 1:
            plan["counts"] = (4 * size["C"], i64)
        self._carve, total = carve(plan)
        self._scarve, stotal = carve({"ranks": (size["rank"], f64), "dense": (size["rank"], i32)})
        self.arena = torch.empty(total, dtype=torch.uint8, device=dev)
        self.scratch = torch.empty(stotal, dtype=torch.uint8, device=dev)
        self.buf = {name: self.arena[a:a + nb].view(dt) for name, (a, nb, dt) in self._carve.items()}
        self.buf.update({name: self.scratch[a:a + nb].view(dt) for name, (a, nb, dt) in self._scarve.items()})

        d = self._d = (_lib.AgreementVideo * n)()
        self._keep = (summaries, scores)
        for v in range(n):
            e = d[v]
            e.user_summary = summaries[v].data_ptr() if self.Us[v] else None
            e.user_scores = scores[v].data_ptr() if self.Uc[v] else None
            e.n_frames, e.n_sum, e.n_sc = self.nf[v], self.Us[v], self.Uc[v]
            e.rank0, e.row0, e.sum0, e.f0, e.c0 = L["rank"][v][0], L["row"][v][0], L["sum"][v][0], L["F"][v][0], L["C"][v][0]
        self._d_dev = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)

    def enqueue(self):
        """sumk_rank_rows -> sumk_agreement_corr and sumk_agreement_f on the current stream (a per-video result no stage owns -- no
        summaries, no scores anywhere in the batch -- is filled with NaN once, at construction time, by `nan_fill`)."""
        lib, b, s = _lib.load(), self.buf, self.size
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        dd, dh = self._d_dev.data_ptr(), C.cast(self._d, C.c_void_p)
        if self.has_corr:
            _lib.check(lib.sumk_rank_rows(dd, dh, self.n, b["ranks"].data_ptr(), b["dense"].data_ptr(), s["rank"], b["ties"].data_ptr(),
                                          b["mean"].data_ptr(), b["ssq"].data_ptr(), s["row"], st), "sumk_rank_rows")
            _lib.check(lib.sumk_agreement_corr(dd, dh, self.n, self._code, b["ranks"].data_ptr(), b["dense"].data_ptr(), s["rank"],
                                               b["ties"].data_ptr(), b["ssq"].data_ptr(), s["row"], b["C"].data_ptr(), s["C"],
                                               b["counts"].data_ptr() if self.metric == 1 else None, b["corr_user"].data_ptr(),
                                               b["corr"].data_ptr(), st), "sumk_agreement_corr")
        if self.has_f:
            _lib.check(lib.sumk_agreement_f(dd, dh, self.n, b["F"].data_ptr(), s["F"], b["f_avg_user"].data_ptr(), b["f_max_user"].data_ptr(),
                                            s["sum"], b["f_avg"].data_ptr(), b["f_max"].data_ptr(), st), "sumk_agreement_f")

    def nan_fill(self):
        """The per-video results of a stage that does not run (NaN): a fill of the chain's own buffers, outside `enqueue()`."""
        if not self.has_corr:
            self.buf["corr"].fill_(float("nan"))
        if not self.has_f:
            self.buf["f_avg"].fill_(float("nan")); self.buf["f_max"].fill_(float("nan"))

    def views(self, buf=None):
        """Per video, the results as views of `buf` (default: the device buffers; `to_host()` for numpy): f_avg, f_max, corr (0-d), f_avg_user,
        f_max_user (Us,), corr_user (Uc,), F (Us, Us), C (Uc, Uc), ties / mean / ssq (Uc,)[, counts (Uc, Uc, 4)]."""
        b, L, out = self.buf if buf is None else buf, self.layout, []
        for v in range(self.n):
            us, uc = self.Us[v], self.Uc[v]
            cut = lambda name, lay, k=1: b[name][k * L[lay][v][0]:k * (L[lay][v][0] + L[lay][v][1])]
            d = {"f_avg": b["f_avg"][v], "f_max": b["f_max"][v], "corr": b["corr"][v], "f_avg_user": cut("f_avg_user", "sum"),
                 "f_max_user": cut("f_max_user", "sum"), "corr_user": cut("corr_user", "row"), "F": cut("F", "F").reshape(us, us),
                 "C": cut("C", "C").reshape(uc, uc), "ties": cut("ties", "row"), "mean": cut("mean", "row"), "ssq": cut("ssq", "row")}
            if self.metric == 1:
                d["counts"] = cut("counts", "C", 4).reshape(uc, uc, 4)
            if buf is None:
                d["ranks"] = cut("ranks", "rank").reshape(uc, self.nf[v]); d["dense"] = cut("dense", "rank").reshape(uc, self.nf[v])
            out.append(d)
        return out

    def to_host(self):
        """ONE D2H of the result arena (synchronises), then numpy views of it keyed like `buf` (the ranks stay on the device)."""
        raw = self.arena.cpu().numpy()
        return {name: raw[a:a + nb].view(_NP[dt]) for name, (a, nb, dt) in self._carve.items()}


def _leaf(x):
    """A numpy array or a device tensor from a record's field: numpy, a tensor, or an h5py-style leaf."""
    if torch.is_tensor(x) or isinstance(x, np.ndarray):
        return x
    return np.asarray(x if isinstance(x, (np.generic, list, tuple)) else x[...])


def _host_rows(key, name, x):
    """One field of one video with every check the host can make; numpy in -> contiguous float32 numpy out, a device tensor stays."""
    if torch.is_tensor(x):
        if x.dim() != 2:
            raise SumkError(f"human_agreement: video {key}: {name} must be (n_users, n_frames), got {tuple(x.shape)}")
        if not x.is_cuda:
            x = x.detach().numpy()
        else:
            return x.detach().to(torch.float32).contiguous()
    x = np.asarray(x)
    if x.ndim != 2:
        raise SumkError(f"human_agreement: video {key}: {name} must be (n_users, n_frames), got {x.shape}")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if not np.all(np.isfinite(x)):
        raise SumkError(f"human_agreement: video {key}: {name} must be finite")
    return x


def _host_corr(x, metric):
    """The correlations of a video past MAX_RANK_FRAMES through the host functions of utils/eval.py: (C, corr_user, corr)."""
    U = x.shape[0]
    C_ = np.array([[ev.evaluate_scores(x[a], x[b:b + 1], metric=metric) for b in range(U)] for a in range(U)], dtype=np.float64).reshape(U, U)
    cu = np.array([np.mean(np.delete(C_[a], a)) if U >= 2 else np.nan for a in range(U)], dtype=np.float64)
    return C_, cu, np.float64(np.mean(cu)) if U >= 2 else np.float64(np.nan)


def _set_mean(values):
    return float(np.mean(values)) if len(values) else float("nan")


def human_agreement(videos, metric="spearmanr", device=False):
    """videos: {key: {user_summary (Us, n_frames) and / or user_scores (Uc, n_frames), ...}} -- a mapping or a `DictDataset`, the fields numpy
    arrays, h5py-style leaves or device tensors (other fields are ignored).  One upload of the batch's inputs (and one of the
    descriptor array), one enqueue of the chain, one D2H.

    Returns {"videos": {key: {f_avg, f_max, corr, f_avg_user, f_max_user, corr_user, F, C, path}}, "corr", "f_avg", "f_max", "result"}:
    per video the leave-one-out means over its annotators (NaN where the input is missing or holds fewer than two annotators), the
    per-annotator vectors and the pairwise matrices; over the set the means of the videos that supplied the input, and `result` =
    (corr, (f_avg, f_max)), the shape of `Trainer.test`.  path: "device", or "host" for a video past MAX_RANK_FRAMES frames, whose
    correlation comes from the host functions of utils/eval.py (its F stays on the device) -- the arrangement `Trainer` has for Kendall.
    device=True: the per-video values stay device tensors (views of the chain's buffers), nothing is copied home and the set-level
    entries are the (n_videos,) device vectors instead of their means; a "host" video's correlation is still computed on the host.
    Raises KeyError for an unknown metric and SumkError -- naming the video and the limit -- for what is past the chain's limits,
    before anything is enqueued; SumkError without a GPU."""
    _metric(metric)
    keys = list(videos.keys())
    if not keys:
        raise SumkError("human_agreement: no videos")
    summ, sc = [], []
    for k in keys:
        rec = videos[k]
        s = _host_rows(k, "user_summary", _leaf(rec["user_summary"])) if "user_summary" in rec else None
        x = _host_rows(k, "user_scores", _leaf(rec["user_scores"])) if "user_scores" in rec else None
        if s is None and x is None:
            raise SumkError(f"human_agreement: video {k} has neither user_summary nor user_scores")
        if s is not None and x is not None and s.shape[1] != x.shape[1]:
            raise SumkError(f"human_agreement: video {k}: user_summary spans {s.shape[1]} frames, user_scores {x.shape[1]}")
        nf = int((s if s is not None else x).shape[1])
        long_ = x is not None and nf > MAX_RANK_FRAMES
        why = refusal(0 if s is None else int(s.shape[0]), 0 if x is None or long_ else int(x.shape[0]), nf)
        if why is None and long_ and x.shape[0] > MAX_USERS:
            why = f"{x.shape[0]} annotators in user_scores (at most {MAX_USERS})"
        if why is not None:
            raise SumkError(f"human_agreement: video {k} has {why}: past the limits of the device chain")
        summ.append(s); sc.append(x)
    if not torch.cuda.is_available():
        raise SumkError("human_agreement: no GPU -- summarizer_amd runs only on the HIP path (no CPU fallback)")
    dev = next((t.device for t in summ + sc if torch.is_tensor(t)), torch.device("cuda", torch.cuda.current_device()))
    # ---- the long videos' scores go to the host functions, everything else up in ONE copy
    host_x = {}
    for i, x in enumerate(sc):
        if x is not None and x.shape[1] > MAX_RANK_FRAMES:
            host_x[i] = x.cpu().numpy() if torch.is_tensor(x) else x
            sc[i] = None
    todo = [(lst, i) for lst in (summ, sc) for i, t in enumerate(lst) if isinstance(t, np.ndarray)]
    if todo:
        total = sum(lst[i].size for lst, i in todo)
        stage = torch.empty(total, dtype=torch.float32).pin_memory()
        flat, at = stage.numpy(), 0
        for lst, i in todo:
            flat[at:at + lst[i].size] = lst[i].reshape(-1); at += lst[i].size
        up, at = stage.to(dev, non_blocking=True), 0
        for lst, i in todo:
            shape, m = lst[i].shape, lst[i].size
            lst[i] = up[at:at + m].view(shape); at += m
    only_host = [i for i in range(len(keys)) if summ[i] is None and sc[i] is None]      # (scores only, past MAX_RANK_FRAMES: nothing for the device)
    live = [i for i in range(len(keys)) if i not in only_host]
    res = [None] * len(keys)
    if live:
        chain = AgreementChain([summ[i] for i in live], [sc[i] for i in live], metric)
        chain.nan_fill()
        chain.enqueue()
        if device:
            views = chain.views()
        else:
            views = chain.views(chain.to_host())
            kernels.health_check()
        for i, r in zip(live, views):
            res[i] = r
    out, names = {}, ("f_avg", "f_max", "corr", "f_avg_user", "f_max_user", "corr_user", "F", "C")
    for i, k in enumerate(keys):
        r = res[i]
        if r is None:
            r = {"f_avg": np.float64(np.nan), "f_max": np.float64(np.nan), "f_avg_user": np.zeros(0, np.float32), "f_max_user": np.zeros(0, np.float32),
                 "F": np.zeros((0, 0), np.float32)}
            if device:
                r = {n_: torch.from_numpy(np.asarray(a)).to(dev) for n_, a in r.items()}
        d = {n_: r[n_] for n_ in names if n_ in r}
        if not device:
            d = {n_: (a.copy() if a.ndim else a[()]) for n_, a in d.items()}
        d["path"] = "device"
        if i in host_x:
            C_, cu, c = _host_corr(host_x[i], metric)
            if device:
                C_, cu, c = (torch.from_numpy(np.asarray(a)).to(dev) for a in (C_, cu, c))
            d.update(C=C_, corr_user=cu, corr=c, path="host")
        out[k] = d
    got = {"videos": out}
    has_f, has_c = [i for i in range(len(keys)) if summ[i] is not None], [i for i in range(len(keys)) if sc[i] is not None or i in host_x]
    if device:
        for name, idx in (("f_avg", has_f), ("f_max", has_f), ("corr", has_c)):
            got[name] = torch.stack([out[keys[i]][name] for i in idx]) if idx else torch.zeros(0, dtype=torch.float64, device=dev)
        got["result"] = None
    else:
        for name, idx in (("f_avg", has_f), ("f_max", has_f), ("corr", has_c)):
            got[name] = _set_mean([out[keys[i]][name] for i in idx])
        got["result"] = (got["corr"], (got["f_avg"], got["f_max"]))
    return got


def rank_users_device(user_scores):
    """`eval.rank_users` on the device (sumk_rank_rows): user_scores (n_users, n_frames) float32, numpy or a device tensor, at most
    MAX_USERS x MAX_RANK_FRAMES.  Returns (ranks, meta): ranks (n_users, n_frames) float64 = rankdata(-user_scores[u]) per row, what
    `eval.rank_users` returns, and the Kendall / Spearman metadata {"dense" (n_users, n_frames) int32, "ties" (n_users,) int64 -- the pair
    `eval_native._kendall_meta` computes -- "mean", "ssq" (n_users,) float64}.  Device tensors for a device tensor, numpy for numpy."""
    on_dev = torch.is_tensor(user_scores) and user_scores.is_cuda
    x = _host_rows("0", "user_scores", user_scores)
    why = refusal(0, int(x.shape[0]), int(x.shape[1]))
    if why is not None:
        raise SumkError(f"rank_users_device: {why}: past the limits of sumk_rank_rows")
    if x.shape[0] == 0:
        raise SumkError("rank_users_device: no rows")
    if not torch.cuda.is_available():
        raise SumkError("rank_users_device: no GPU -- summarizer_amd runs only on the HIP path (no CPU fallback)")
    if not on_dev:
        x = torch.from_numpy(x).to(torch.device("cuda", torch.cuda.current_device()))
    chain = AgreementChain([None], [x], "spearmanr")
    lib, b, s = _lib.load(), chain.buf, chain.size
    _lib.check(lib.sumk_rank_rows(chain._d_dev.data_ptr(), C.cast(chain._d, C.c_void_p), 1, b["ranks"].data_ptr(), b["dense"].data_ptr(), s["rank"],
                                  b["ties"].data_ptr(), b["mean"].data_ptr(), b["ssq"].data_ptr(), s["row"],
                                  C.c_void_p(torch.cuda.current_stream(chain.device).cuda_stream)), "sumk_rank_rows")
    r = chain.views()[0]
    ranks, meta = r["ranks"], {"dense": r["dense"], "ties": r["ties"], "mean": r["mean"], "ssq": r["ssq"]}
    if on_dev:
        return ranks, meta
    out = ranks.cpu().numpy(), {k: t.cpu().numpy() for k, t in meta.items()}
    kernels.health_check()
    return out


def table_row(got, metric="spearmanr"):
    """The "human" row of the baseline table: mean F (avg), mean F (max) and mean correlation over the set."""
    return f"human  F-avg {got['f_avg']:.4f}  F-max {got['f_max']:.4f}  {metric} {got['corr']:.4f}  ({len(got['videos'])} videos)"


def main(argv=None):
    """python -m summarizer_amd.utils.agreement DATA.npz [--metric spearmanr|kendalltau]: DATA holds "<video>/<field>" arrays with
    user_summary and / or user_scores per video (a dataset file `open_dataset` reads); prints the human row of the baseline table."""
    import argparse
    from .datasets import DictDataset
    ap = argparse.ArgumentParser(prog="python -m summarizer_amd.utils.agreement", description=main.__doc__)
    ap.add_argument("data")
    ap.add_argument("--metric", choices=sorted(METRICS), default="spearmanr")
    a = ap.parse_args(argv)
    src = DictDataset.from_npz(a.data)
    videos = {k: {f: g[f][...] for f in ("user_summary", "user_scores") if f in g} for k, g in src.items()}
    print(table_row(human_agreement(videos, a.metric), a.metric))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
