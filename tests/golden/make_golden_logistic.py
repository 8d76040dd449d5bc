#!/usr/bin/env python3
"""Goldens of the two baselines from the REAL reference (summarizer/models/logistic.py, rand.py), under the same stand-ins as
make_golden_e2e.py (in-memory h5py, no OR-tools: selection_algorithm="rank").
  logistic.npz      LogisticRegression eval outputs (D = 64, 128; T in {1, 2, 37, 300}; B in {1, 3}; inputs by recipe), the seeded
                    initial weights (D = 64, 128 as arrays; D = 1024 as the sha256 of each state_dict tensor, plus y on a recipe input),
                    3 steps of nn.MSELoss + Adam(lr, wd) on one video and on a 2-video batch (mean of the per-video losses), and draws
                    of the reference's Random module.
  e2e_logistic.npz  LogisticRegressionTrainer reset -> train -> test on a synthetic dataset (per-epoch losses, weights, metrics).
  e2e_random.npz    RandomTrainer the same way (losses, last-epoch training scores, metrics).
Run once in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_logistic.py"""
import os, sys, types, random
import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"; sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
from summarizer_amd.utils.datasets import synthetic_dataset
from summarizer_amd.utils.hps import make_hps
import recipes as R

DS = {}
h5 = types.ModuleType("h5py")
h5.File = lambda path, mode="r": DS[path]
sys.modules["h5py"] = h5
for name in ["ortools", "ortools.algorithms", "ortools.algorithms.pywrapknapsack_solver"]:
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["ortools.algorithms"].pywrapknapsack_solver = sys.modules["ortools.algorithms.pywrapknapsack_solver"]
sys.path.insert(0, "/root/reference")
import torch
from summarizer.models.logistic import LogisticRegression, LogisticRegressionTrainer
from summarizer.models.rand import Random, RandomTrainer

torch.set_num_threads(4)

# ---------------------------------------------------------------- logistic.npz
out = {}
for D in (64, 128):
    torch.manual_seed(1000 + D)
    m = LogisticRegression(input_size=D).eval()
    for k, v in m.state_dict().items():
        out[f"D{D}/w0/{k}"] = v.numpy().copy()
    for T in (1, 2, 37, 300):
        for B in (1, 3):
            x = R.features(T, B, D, 10 * T + B)
            with torch.no_grad():
                out[f"D{D}/T{T}B{B}/y"] = m(torch.from_numpy(x)).numpy()
torch.manual_seed(2024)
m = LogisticRegression()
sd = m.state_dict()
out["D1024/seed"] = np.array([2024])
out["D1024/keys"] = np.array(list(sd))
out["D1024/sha"] = np.array([R.digest({k: sd[k].numpy()}) for k in sd])
with torch.no_grad():
    out["D1024/y"] = m.eval()(torch.from_numpy(R.features(50, 1, 1024, 3))).numpy()

LR, WD, DT = 1e-2, 1e-5, 128
for name, lens in (("one", (37,)), ("two", (37, 50))):
    torch.manual_seed(7)
    m = LogisticRegression(input_size=DT)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    crit = torch.nn.MSELoss()
    vids = [R.synthetic_video(T, 40 + i, n_users=2, D=DT) for i, T in enumerate(lens)]
    for s in range(3):
        loss = 0
        for v in vids:
            x = torch.from_numpy(v["features"]).unsqueeze(1)
            t = torch.from_numpy(v["gtscore"].copy()).view(-1, 1, 1)
            t -= t.min(); t /= t.max() - t.min()
            loss = loss + crit(m(x), t) / len(vids)
        opt.zero_grad(); loss.backward(); opt.step()
        out[f"traj/{name}/loss{s}"] = np.array([float(loss.detach())], dtype=np.float32)
        for k, v in m.state_dict().items():
            out[f"traj/{name}/w{s}/{k}"] = v.numpy().copy()
    out[f"traj/{name}/lens"] = np.array(lens)
out["traj/meta"] = np.array([LR, WD, DT], dtype=np.float64)

torch.manual_seed(99)
out["random/y"] = Random()(torch.zeros(37, 3, 8)).numpy()
np.savez_compressed(os.path.join(HERE, "logistic.npz"), **out)


# ---------------------------------------------------------------- e2e_logistic.npz / e2e_random.npz
def run(trainer_cls, fname, D=128, SEED=31, n=11, dseed=6, t0=40, t1=90, nu=6, epochs=3):
    ds = synthetic_dataset(n, seed=dseed, D=D, t_range=(t0, t1), n_users=nu)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
    DS["synthetic.h5"] = ds
    hps = make_hps("synthetic.h5", [{"train_keys": keys[3:], "test_keys": keys[:3]}], epochs=epochs, test_every_epochs=1, lr=1e-3,
                   use_cuda=False, selection_algorithm="rank", extra_params={})
    got = {}

    class RefTrainer(trainer_cls):
        def _init_model(self):
            return LogisticRegression(input_size=D) if trainer_cls is LogisticRegressionTrainer else Random()

        def draw_scores(self, fold, dist_scores):
            got.update(dist_scores)
            super().draw_scores(fold, dist_scores)

    torch.manual_seed(SEED); random.seed(SEED)
    tr = RefTrainer(hps, hps.splits_files[0]).reset()
    res = {f"w0/{k}": v.detach().numpy().copy() for k, v in tr.model.state_dict().items()}
    best = tr.train(0)
    res.update({f"w1/{k}": v.detach().numpy().copy() for k, v in tr.model.state_dict().items()})
    for tag, key in (("losses", "Train/Loss"), ("corr", "Test/Correlation"), ("f_avg", "Test/F-score_avg"), ("f_max", "Test/F-score_max")):
        res[tag] = np.array([v for _, v in hps.writer.scalars[f"synthetic/Fold_1/{key}"]], dtype=np.float64)
    res["best"] = np.array(best, dtype=np.float64)
    for k, v in got.items():
        res[f"train_scores/{k}"] = np.asarray(v).reshape(-1)
    res["meta"] = np.array([D, SEED, n, dseed, t0, t1, nu, epochs])
    np.savez_compressed(os.path.join(HERE, fname), **res)
    print(fname, "losses", res["losses"], "corr", res["corr"], "f", res["f_avg"], res["f_max"], "best", best)


run(LogisticRegressionTrainer, "e2e_logistic.npz")
run(RandomTrainer, "e2e_random.npz")
for f in ("logistic.npz", "e2e_logistic.npz", "e2e_random.npz"):
    print(f, os.path.getsize(os.path.join(HERE, f)) / 1024, "KB")
