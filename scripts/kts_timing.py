"""Change points on the device (sumk_kts, csrc/kts.hip) beside the float64 numpy reference on the host (tests/kts_ref.py), on
  * the 50-video S-TVSum batch shape (videos of 150 .. 320 steps, 11 941 steps in all, D = 1024), max_ncp = the default min(n - 1, 1023): ONE call for the batch;
  * one n = 1024 video (D = 1024), max_ncp = 1023 -- the dynamic programme at its densest -- and max_ncp = 40.
Rows are L2-normalised planted segments (tests/kts_ref.planted_features), as the tests use.  The device figure is the median over
repeated calls of one call's stream time (HIP events around the call; warm-up first); the host figure is one run of the reference on a
few videos of the batch (its per-video mean is extrapolated to 50) and on the n = 1024 video.  The measuring process is a child of this
script and runs under a time limit, so a hang ends it:
    python scripts/kts_timing.py [OUT.json]                 (prints the JSON record; the figures in DESIGN.md are such a record)
    rocprofv3 --kernel-trace --stats ... -- python scripts/kts_timing.py trace      (the five launches of a call, per kernel)"""
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420


def worker(mode):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kts_ref
    from summarizer_amd import kernels
    from summarizer_amd.utils import kts
    dev = torch.device("cuda:0")
    from summarizer_amd.utils.datasets import synthetic_dataset
    ds = synthetic_dataset(50, seed=11, D=16, t_range=(150, 320), n_users=1)          # the S-TVSum lengths (the features are replaced)
    lens = [int(ds[k]["features"].shape[0]) for k in ds.keys()]
    feats = [kts_ref.planted_features(n, 1024, max(2, n // 30), 0.3, 500 + i)[0] for i, n in enumerate(lens)]
    long_x = kts_ref.planted_features(1024, 1024, 30, 0.3, 77)[0]

    def device_ms(x, ls, max_ncp, reps):
        sb = kernels.SeqBatch.get(ls, dev)
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        for _ in range(3):
            out = kernels.kts(xd, sb, max_ncp, want_scores=False)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = kernels.kts(xd, sb, max_ncp, want_scores=False); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), [round(t, 4) for t in ts], out

    batch_ncp = kts.default_max_ncp(max(lens))
    if mode == "trace":
        device_ms(np.concatenate(feats), lens, batch_ncp, 5)
        device_ms(long_x, [1024], 1023, 3)
        return
    rec = {"box": "1x MI355X", "date": time.strftime("%Y-%m-%d"), "D": 1024}
    ms, all_ms, out = device_ms(np.concatenate(feats), lens, batch_ncp, 10)
    n_cps = out[0].cpu().numpy()
    pairs = sum(min(batch_ncp, n - 1) * (n + 1) * n // 2 for n in lens)
    rec["batch"] = {"videos": 50, "steps": sum(lens), "max_ncp": batch_ncp, "device_ms": ms, "device_ms_all": all_ms, "dp_pairs_upper_bound": pairs,
                    "n_cps_mean": float(n_cps.mean())}
    t0 = time.perf_counter()
    sub = 3
    for i in range(sub):
        X = feats[i].astype(np.float64)
        ref = kts_ref.cpd_auto(X @ X.T, min(batch_ncp, lens[i] - 1), full=True)
        assert ref[0] == n_cps[i], (i, ref[0], n_cps[i])
    host = (time.perf_counter() - t0) / sub
    rec["batch"]["host_numpy_s_per_video"] = host
    rec["batch"]["host_numpy_s_extrapolated_50"] = host * 50
    for ncp, reps in ((1023, 5), (40, 10)):
        ms, all_ms, out = device_ms(long_x, [1024], ncp, reps)
        e = {"n": 1024, "max_ncp": ncp, "device_ms": ms, "device_ms_all": all_ms, "n_cps": int(out[0][0]), "dp_pairs": ncp * 1025 * 1024 // 2}
        e["dp_bytes_of_J_per_s"] = e["dp_pairs"] * 8 / (ms * 1e-3)
        X = long_x.astype(np.float64)
        t0 = time.perf_counter()
        ref = kts_ref.cpd_auto(X @ X.T, ncp, full=True)
        e["host_numpy_s"] = time.perf_counter() - t0
        assert ref[0] == e["n_cps"]
        rec[f"single_n1024_ncp{ncp}"] = e
    line = json.dumps(rec)
    print("KTS-TIMING", line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "worker":
        worker(sys.argv[2])
    else:
        mode = "trace" if len(sys.argv) > 1 and sys.argv[1] == "trace" else "time"
        out = [a for a in sys.argv[1:] if a.endswith(".json")][:1]
        # a fresh child does the GPU work (this process never opens the device) under a time limit of its own
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "worker", mode] + out, timeout=LIMIT_S).returncode)
