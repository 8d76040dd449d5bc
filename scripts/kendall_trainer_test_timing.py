"""Trainer.test on the 50-video S-TVSum-shaped set (bench.trainer_test_leg's set-up): Spearman, Kendall through scipy, Kendall through the
device kernel, Kendall through the native host threads.  Alternating rounds; medians and every round's figure go to the JSON file named
by the second argument (the record under profiles/ is such a file).
    python scripts/kendall_trainer_test_timing.py time OUT.json
    rocprofv3 --kernel-trace --stats ... -- python scripts/kendall_trainer_test_timing.py trace      (the Kendall launch alone)"""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summarizer_amd.models.vasnet import VASNetTrainer
from summarizer_amd.utils.datasets import synthetic_dataset
from summarizer_amd.utils.hps import make_hps
from summarizer_amd.utils import eval_native

mode = sys.argv[1] if len(sys.argv) > 1 else "time"
ds = synthetic_dataset(50, seed=11, D=1024, t_range=(150, 320), n_users=20)
keys = list(ds.keys())
hps = make_hps(ds, [{"train_keys": [], "test_keys": keys}], epochs=1, extra_params={})
torch.manual_seed(1234)
tr = VASNetTrainer(hps, hps.splits_files[0]).reset()
frames = int(sum(int(ds[k]["n_frames"][()]) for k in keys))

def run(metric, n):
    tr.hps.correlation_metric = metric
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        res = tr.test(0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, res

def scipy_path():
    tr.hps.correlation_metric = "kendalltau"
    tr.model.eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        act = tr._score_keys(keys)
    corr = tr._eval_scores(act, keys)
    tr.hps.correlation_metric = "spearmanr"
    f = tr._evaluate_native(act, keys)
    return (time.perf_counter() - t0) * 1e3, corr

if mode == "trace":            # for the kernel trace: a few Kendall calls only
    run("kendalltau", 3); run("kendalltau", 20)
    sys.exit(0)

for m in ("spearmanr", "kendalltau"):
    run(m, 10)
out = dict(spearman_ms=[], kendall_device_ms=[], kendall_host_ms=[], kendall_scipy_ms=[])
for r in range(5):
    out["spearman_ms"].append(run("spearmanr", 100)[0])
    t, dev_res = run("kendalltau", 100)
    out["kendall_device_ms"].append(t)
sc = [scipy_path() for _ in range(2)]
out["kendall_scipy_ms"] = [s[0] for s in sc]
# the native host tail on the same set: every video marked as not qualifying for the device tail
for k in keys:
    tr._native_meta(k)["_dev_ready"] = False
run("kendalltau", 5)
for r in range(5):
    t, host_res = run("kendalltau", 30)
    out["kendall_host_ms"].append(t)
out["results"] = dict(device=[float(dev_res[0]), float(dev_res[1][0]), float(dev_res[1][1])], host=[float(host_res[0]), float(host_res[1][0]), float(host_res[1][1])],
                      scipy_corr=float(sc[0][1]))
out["device_equals_host"] = bool(dev_res == host_res)
out["frames"] = frames
out["median"] = {k: float(np.median(v)) for k, v in out.items() if k.endswith("_ms")}
dest = sys.argv[2] if len(sys.argv) > 2 else "kendall_trainer_test.json"
json.dump(out, open(dest, "w"), indent=1)
print(json.dumps(out["median"]), out["device_equals_host"], out["results"])
