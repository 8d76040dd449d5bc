#!/usr/bin/env python3
"""Golden of the inter-annotator agreement specification (tests/agreement_ref.py) from the REAL reference's `evaluate_summary` and
`evaluate_scores` (summarizer/utils/eval.py:49-72, 125-165), imported under the usual stand-ins for h5py / ortools.  One synthetic video,
U = 5 annotators, 611 frames:
  - the inputs (user_summary: 0 / positive marks; user_scores: grades 1 .. 5 rescaled to [0, 1]);
  - leave-one-out: evaluate_summary(user_summary[a], the other rows) -> (avg, max) per annotator; evaluate_scores(user_scores[a], the
    other rows, metric) per annotator, both metrics;
  - every pairwise value from single-row calls: evaluate_summary(us[a], us[b:b+1])[0] and evaluate_scores(sc[a], sc[b:b+1], metric).
Seeds are drawn until (1) every pair of annotators overlaps in at least one frame -- otherwise the reference's python-float `0.` branch
turns its mean into float64, a quirk the package's tail does not carry -- and (2) no score row is constant; both are asserted.
Run once in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_agreement.py"""
import os, sys, types
import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
for name in ["h5py", "ortools", "ortools.algorithms", "ortools.algorithms.pywrapknapsack_solver"]:
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["ortools.algorithms"].pywrapknapsack_solver = sys.modules["ortools.algorithms.pywrapknapsack_solver"]
sys.path.insert(0, "/root/reference")

from summarizer.utils import eval as ref_eval

U, n_frames = 5, 611


def overlaps(us):
    on = us > 0
    return all((on[a] & on[b]).any() for a in range(U) for b in range(U))


for seed in range(20250, 20350):
    rng = np.random.default_rng(seed)
    user_summary = ((rng.random((U, n_frames)) < 0.2) * rng.integers(1, 4, size=(U, n_frames))).astype(np.float32)
    user_scores = ((rng.integers(1, 6, size=(U, n_frames)).astype(np.float32) - np.float32(1)) / np.float32(4)).astype(np.float32)
    if overlaps(user_summary) and all(np.unique(user_scores[u]).size > 1 for u in range(U)):
        break
else:
    raise SystemExit("no draw with overlapping summaries and non-constant scores")
assert overlaps(user_summary)
assert all(user_scores[u].min() != user_scores[u].max() for u in range(U))

out = {"seed": np.int64(seed), "user_summary": user_summary, "user_scores": user_scores}
others = lambda a: [b for b in range(U) if b != a]
loo = [ref_eval.evaluate_summary(user_summary[a].copy(), user_summary[others(a)].copy()) for a in range(U)]
assert all(isinstance(v, np.float32) for pair in loo for v in pair), "the reference's mean left float32: a pair without overlap"
out["f_avg_user"] = np.array([p[0] for p in loo], dtype=np.float32)
out["f_max_user"] = np.array([p[1] for p in loo], dtype=np.float32)
F = [[ref_eval.evaluate_summary(user_summary[a].copy(), user_summary[b:b + 1].copy())[0] for b in range(U)] for a in range(U)]
assert all(isinstance(v, np.float32) for row in F for v in row)
out["F"] = np.array(F, dtype=np.float32)
for metric in ("spearmanr", "kendalltau"):
    out[f"{metric}/corr_user"] = np.array([ref_eval.evaluate_scores(user_scores[a], user_scores[others(a)], metric) for a in range(U)], dtype=np.float64)
    out[f"{metric}/C"] = np.array([[ref_eval.evaluate_scores(user_scores[a], user_scores[b:b + 1], metric) for b in range(U)] for a in range(U)],
                                  dtype=np.float64)
path = os.path.join(HERE, "agreement.npz")
np.savez_compressed(path, **out)
print(f"agreement: seed {seed}, {U} annotators, {n_frames} frames, F in [{out['F'].min():.3f}, {out['F'].max():.3f}], "
      f"rho mean {out['spearmanr/corr_user'].mean():.4f}, tau mean {out['kendalltau/corr_user'].mean():.4f}, {os.path.getsize(path) / 1024:.1f} KB")
