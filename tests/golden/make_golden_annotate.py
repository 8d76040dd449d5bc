#!/usr/bin/env python3
"""Golden of the dataset-record specification (tests/annotate_ref.py) from the REAL reference's `upsample` and
`generate_summary(method="rank")` (summarizer/utils/eval.py:15-35, 74-123), imported under the usual stand-ins for h5py / ortools:
  - the protocol-"summaries" `user_scores` row: the reference's upsample of the selection frequency at the picks;
  - rank-mode `user_summary` (one row per annotator, positions = arange(n_frames)) and `gtsummary` of one synthetic video, for both
    protocols' gtscore.
The frame-level arithmetic in front (user_scores, consensus, gtscore) is annotate_ref's own -- the reference has no code for it
(summarizer/datasets/README.md:50-74 describes it in words).  The video is drawn so that NO two segment scores are equal: the
reference's `np.argsort(seg_score)[::-1]` is then one order on every machine.  The knapsack stays pinned to the project's host DP
(tests/golden/knapsack_e2e.npz), as everywhere else.
Run once in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_annotate.py"""
import os, sys, types
import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
for name in ["h5py", "ortools", "ortools.algorithms", "ortools.algorithms.pywrapknapsack_solver"]:
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["ortools.algorithms"].pywrapknapsack_solver = sys.modules["ortools.algorithms.pywrapknapsack_solver"]
sys.path.insert(0, "/root/reference")

from summarizer.utils import eval as ref_eval
import annotate_ref as A

U, n_frames = 5, 611
lengths = [1, 7, 8, 9, 128, 129, 61, 40, 97, 23, 57, 51]
assert sum(lengths) == n_frames
cps, nfps = A.segments_of_lengths(lengths)
picks = np.arange(0, n_frames - 5, 15).astype(np.int32)           # the last pick is short of n_frames - 1


def untied(scores, positions):
    frame = ref_eval.upsample(scores, n_frames, positions)
    means = [float(frame[lo:hi + 1].mean()) for lo, hi in cps]
    return len(set(means)) == len(means)


for seed in range(20240, 20340):                                  # the first draw without equal segment scores anywhere
    rng = np.random.default_rng(seed)
    anno_scores = rng.integers(1, 6, size=(U, n_frames)).astype(np.float32)
    anno_summaries = ((rng.random((U, n_frames)) < 0.3) * rng.integers(1, 4, size=(U, n_frames))).astype(np.float32)
    fs, fm = A.scores_frame_level(anno_scores, picks, cps), A.summaries_frame_level(anno_summaries, picks)
    if (all(untied(fs["user_scores"][u], np.arange(n_frames)) for u in range(U)) and untied(fs["gtscore"], picks)
            and untied(fm["gtscore"], picks)):
        break
else:
    raise SystemExit("no draw without ties")

out = {"seed": np.int64(seed), "n_frames": np.int64(n_frames), "picks": picks, "change_points": cps, "n_frame_per_seg": nfps, "anno_scores": anno_scores,
       "anno_summaries": anno_summaries}
fl = A.scores_frame_level(anno_scores, picks, cps)
rows = []
for u in range(U):
    rows.append(ref_eval.generate_summary(fl["user_scores"][u], cps, n_frames, nfps.tolist(), np.arange(n_frames), 0.15, "rank"))
out["scores/user_summary_rank"] = np.stack(rows).astype(np.float32)
out["scores/gtsummary_rank"] = ref_eval.generate_summary(fl["gtscore"], cps, n_frames, nfps.tolist(), picks, 0.15, "rank")[picks].astype(np.float32)
fl = A.summaries_frame_level(anno_summaries, picks)
out["summaries/user_scores"] = np.asarray(ref_eval.upsample(fl["gtscore"], n_frames, picks), dtype=np.float32)[None, :]
out["summaries/gtsummary_rank"] = ref_eval.generate_summary(fl["gtscore"], cps, n_frames, nfps.tolist(), picks, 0.15, "rank")[picks].astype(np.float32)
path = os.path.join(HERE, "annotate.npz")
np.savez_compressed(path, **out)
print(f"annotate: {U} annotators, {n_frames} frames, {len(lengths)} segments, rank summaries select "
      f"{int(out['scores/user_summary_rank'].sum())} + {int(out['scores/gtsummary_rank'].sum())} + {int(out['summaries/gtsummary_rank'].sum())}, "
      f"{os.path.getsize(path) / 1024:.1f} KB")
