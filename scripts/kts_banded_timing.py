"""Banded, chip-wide KTS (sumk_kts_banded, csrc/kts_banded.hip) beside the dense path (sumk_kts, csrc/kts.hip) on one long video.

The yardstick is the dense path on the same inputs and box.  It is timed first at n = 2048, max_ncp = 40; that time, scaled by n^2 m, is the
estimate for n = 4096, 8192, 16384 at max_ncp = 40, and a size is run only where warm-up + repeats fit half of the step's time limit (the
skipped sizes and the estimate that skipped them are recorded).  The banded path is then timed
  * at the shapes of the dense runs (lmax = the default 100000, so B = n and both paths return the same bits: checked);
  * at the default max_ncp = 1023 for n = 8192 and 16384 (estimated from the bytes/s of the previous banded step; skipped where it does not fit);
  * past the dense cap: n = 65536, D = 1024, lmax = 2048, max_ncp = 1023 -- about 1.1 GB of band -- and n = 20000 with the whole triangle
    (lmax = the default, B = n: 3.2 GB of band behind 1.6 GB of Gram strips), max_ncp = 200; in both the planted boundaries must come back.
    In this layout the n = 65536 workspace is 1.63 GB, so every offset of that run stays BELOW 2^31 bytes; the n = 20000 run is the one
    whose offsets pass 2^31 (and 2^32) bytes, as tests/test_gpu_kts_banded.py::test_offsets_past_2_31_bytes does at D = 64.
Per run: the median over repeated calls of one call's stream time (HIP events around the call, warm-up first; a run estimated above 20 s is
timed ONCE, without warm-up, and says so), the bytes of J the dynamic programme streams per second (8 bytes per (t, l) pair of all rows
run), and the ratio to the dense time where both ran.  D = 1024, rows are L2-normalised planted segments.  Every GPU step is a fresh child of
this script under its own time limit; after a step that fails or runs out of time nothing more is started.
    python scripts/kts_banded_timing.py [OUT.json] [--steps=dense,banded,default,wide,long]      (writes profiles/kts_banded_timing.json by default)"""
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 1024
STEP_LIMIT_S = 300
LONG_LIMIT_S = 1000
BASE_N, BASE_M = 2048, 40


def dp_pairs(n, m, lmin, lmax):
    """(t, l) pairs the DP rows 1 .. m read: one float64 of J each."""
    import numpy as np
    total = 0
    for k in range(1, m + 1):
        lo = (k + 1) * lmin
        if lo > n:
            break
        l = np.arange(lo, n + 1, dtype=np.int64)
        total += int((l - np.maximum(k * lmin, l - lmax)).sum())
    return total


def planted(n, seg_lo, seg_hi, seed):
    """float32 (n, D) rows: piecewise-constant means + 0.3 noise, L2-normalised; segment lengths uniform in seg_lo .. seg_hi."""
    import numpy as np
    rng = np.random.default_rng(seed)
    bounds, at = [], 0
    while True:
        at += int(rng.integers(seg_lo, seg_hi + 1))
        if at > n - seg_lo:
            break
        bounds.append(at)
    bounds = np.array(bounds, dtype=np.int64)
    X = np.empty((n, D), dtype=np.float32)
    for a, b in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [n]])):
        X[a:b] = rng.standard_normal(D).astype(np.float32) + 0.3 * rng.standard_normal((b - a, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X, bounds


def worker(spec):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from summarizer_amd import kernels
    dev = torch.device("cuda:0")
    n, m, lmax, reps, warm = spec["n"], spec["max_ncp"], spec["lmax"], spec["reps"], spec["warmup"]
    X, bounds = planted(n, spec["seg_lo"], spec["seg_hi"], 1000 + n)
    xd = torch.from_numpy(X).to(dev)
    sb = kernels.SeqBatch.get([n], dev)
    out = {"n": n, "max_ncp": m, "lmax": lmax, "B": min(lmax, n), "reps": reps, "warmup": warm}

    def timed(fn):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); res = fn(); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), [round(t, 3) for t in ts], res

    pairs = dp_pairs(n, m, 1, lmax)
    out["dp_pairs"] = pairs
    res = {}
    for path in spec["paths"]:
        if path == "dense":
            out["dense_workspace_bytes"] = kernels.kts_workspace_bytes(D, sb, m)
            ms, all_ms, res[path] = timed(lambda: kernels.kts(xd, sb, m, lmax=lmax))
        else:
            out["banded_workspace_bytes"] = kernels.kts_banded_workspace_bytes(D, sb, m, lmax)
            ms, all_ms, res[path] = timed(lambda: kernels.kts_banded(xd, sb, m, lmax=lmax))
        out[path + "_ms"], out[path + "_ms_all"] = ms, all_ms
        out[path + "_J_bytes_per_s"] = pairs * 8 / (ms * 1e-3)
    if len(res) == 2:
        a, b = res["dense"], res["banded"]
        out["same_bits"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int64), b[2].view(torch.int64)))
        out["banded_over_dense"] = out["banded_ms"] / out["dense_ms"]
    r = res.get("banded", res.get("dense"))
    k = int(r[0][0])
    cps = r[1][0, :k].cpu().numpy()
    out["n_cps"], out["planted"] = k, int(len(bounds))
    out["planted_boundaries_returned"] = bool(k == len(bounds) and np.array_equal(cps, bounds))
    out["planted_boundaries_found"] = int(np.isin(bounds, cps).sum())
    print("KTS-BANDED-STEP", json.dumps(out), flush=True)


def run_step(spec, limit):
    """A fresh child does the GPU work of one step under its own time limit; None = it failed or ran out of time."""
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", json.dumps(spec)], timeout=limit, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        print(f"step {spec} ran past its limit of {limit} s", flush=True)
        return None
    for line in p.stdout.splitlines():
        if line.startswith("KTS-BANDED-STEP "):
            print(line, flush=True)
            return json.loads(line[len("KTS-BANDED-STEP "):])
    print(f"step {spec} failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
    return None


def plan(est_s, limit):
    """(warm-up, repeats) for a call estimated at est_s seconds, or None when even one call does not fit half the step's limit."""
    if est_s > 0.5 * limit:
        return None
    if est_s > 20:
        return 0, 1
    reps = 5 if 6 * est_s <= 0.5 * limit else 3 if 4 * est_s <= 0.5 * limit else 1
    return 1, reps


def main(argv):
    out_path = next((a for a in argv if a.endswith(".json")), os.path.join(ROOT, "profiles", "kts_banded_timing.json"))
    steps = next((a.split("=", 1)[1] for a in argv if a.startswith("--steps=")), "dense,banded,default,wide,long").split(",")
    rec = {"box": "1x MI355X", "D": D, "runs": {}, "skipped": {}}          # every run carries its own date: a partial re-run merges into the record
    if os.path.exists(out_path):
        with open(out_path) as f:
            old = json.loads(f.read())
        rec["runs"], rec["skipped"] = old.get("runs", {}), old.get("skipped", {})
        for r in rec["runs"].values():
            r.setdefault("date", old.get("date", "unknown"))
    runs, skipped = rec["runs"], rec["skipped"]

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")

    def step(tag, spec, limit):
        spec = dict({"lmax": 100000, "seg_lo": 60, "seg_hi": 400}, **spec)
        r = run_step(spec, limit)
        if r is None:
            save()
            sys.exit(f"{tag}: the step failed or ran out of time -- nothing more is started")
        runs[tag] = dict(runs.get(tag, {}), date=time.strftime("%Y-%m-%d"), **r)
        skipped.pop(tag, None)
        save()
        return runs[tag]

    scale = lambda n, m: (n / BASE_N) ** 2 * (m / BASE_M)
    if "dense" in steps:
        base = step(f"n{BASE_N}_ncp{BASE_M}", {"n": BASE_N, "max_ncp": BASE_M, "paths": ["dense", "banded"], "reps": 5, "warmup": 1}, STEP_LIMIT_S)
        for n in (4096, 8192, 16384):
            tag, est = f"n{n}_ncp{BASE_M}", base["dense_ms"] * 1e-3 * scale(n, BASE_M)
            pl = plan(est, STEP_LIMIT_S)
            if pl is None:
                skipped[tag + "_dense"] = f"dense estimate {est:.1f} s per call (n^2 m scaling of n={BASE_N}) does not fit half of the {STEP_LIMIT_S} s step limit"
                save()
                continue
            step(tag, {"n": n, "max_ncp": BASE_M, "paths": ["dense"], "reps": pl[1], "warmup": pl[0]}, STEP_LIMIT_S)
    if "banded" in steps:
        for n in (4096, 8192, 16384):
            tag = f"n{n}_ncp{BASE_M}"
            r = step(tag, {"n": n, "max_ncp": BASE_M, "paths": ["banded"], "reps": 5, "warmup": 1}, STEP_LIMIT_S)
            if "dense_ms" in r:
                r["banded_over_dense"] = r["banded_ms"] / r["dense_ms"]
                save()
    rate = max((r["banded_J_bytes_per_s"] for r in runs.values() if "banded_J_bytes_per_s" in r and r["n"] >= 8192), default=None)
    if rate is None and ("default" in steps or "long" in steps):
        sys.exit("the default / long steps are sized from the bytes/s of a banded run with n >= 8192: run the `banded` (or `wide`) step first")
    if "default" in steps:
        for n in (8192, 16384):
            tag = f"n{n}_ncp1023"
            est = dp_pairs(n, 1023, 1, 100000) * 8 / rate if rate else float("inf")
            pl = plan(est, STEP_LIMIT_S)
            if pl is None:
                skipped[tag] = f"banded estimate {est:.1f} s per call (bytes of J at {rate:.3g} B/s) does not fit half of the {STEP_LIMIT_S} s step limit"
                save()
                continue
            step(tag, {"n": n, "max_ncp": 1023, "paths": ["banded"], "reps": pl[1], "warmup": pl[0]}, STEP_LIMIT_S)
    if "wide" in steps:
        r = step("n20000_full_ncp200", {"n": 20000, "max_ncp": 200, "paths": ["banded"], "reps": 3, "warmup": 1}, STEP_LIMIT_S)
        r["note"] = "B = n: band offsets past 2^31 and 2^32 bytes"
        save()
        if not r["planted_boundaries_returned"]:
            sys.exit("n = 20000: the planted boundaries did not come back")
    if "long" in steps:
        n, lmax, tag = 65536, 2048, "n65536_lmax2048_ncp1023"
        est = dp_pairs(n, 1023, 1, lmax) * 8 / rate if rate else float("inf")
        pl = plan(est, LONG_LIMIT_S)
        if pl is None:
            skipped[tag] = f"banded estimate {est:.1f} s per call (bytes of J at {rate:.3g} B/s) does not fit half of the {LONG_LIMIT_S} s step limit"
        else:
            r = step(tag, {"n": n, "max_ncp": 1023, "lmax": lmax, "seg_lo": 200, "seg_hi": 1200, "paths": ["banded"], "reps": pl[1], "warmup": pl[0]},
                     LONG_LIMIT_S)
            r["note"] = "past the dense cap; workspace 1.63 GB: every offset below 2^31 bytes"
            save()
            if not r["planted_boundaries_returned"]:
                sys.exit("n = 65536: the planted boundaries did not come back")
        save()
    print("KTS-BANDED-TIMING", json.dumps(rec))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "worker":
        worker(json.loads(sys.argv[2]))
    else:
        main(sys.argv[1:])
