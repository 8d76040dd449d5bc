"""The DSN reward on the streaming path (kernels.dsn_reward(..., path="stream"), csrc/reward_stream.hip) beside the Gram path on long videos.

D = 1024, E = 5 episodes, the default temporal threshold (20), pick rate 0.5, exact fp32:
  * a Twitch-LOL-shaped batch, 8 videos of 3600 to 7200 steps: both paths;
  * one video of T = 16384: both paths;
  * one video of T = 65536: the stream path alone.  The Gram run is skipped there -- its workspace query answers more than GRAM_MAX_WS (the
    Gram matrix alone is 17.2 GB) -- and the record says so with the bytes it asked for: not run, not estimated;
  * at T = 65536 the launches of the stream path separately (event pairs of the library's profiler around each).
Expectation, recorded beside each measurement: 2 T^2 D FLOP per video at the rate the lean fp32 MFMA kernel reaches in the band products
(about 117 TFLOP/s, README) -- about 75 ms at T = 65536.  That rate was measured on the band products, not on this kernel.  The one
condition: at T = 16384 the stream path is not slower than the Gram path in the same run ("stream_not_slower"): it does the same FLOPs
without the 1 GB store and the five 1 GB reads.
Per run: the median over 5 calls of one call's stream time (HIP events around the call, 2 warm-up calls first).  Every GPU step is a fresh
child of this script under its own time limit; after a step that fails or runs out of time nothing more is started.
    python scripts/reward_stream_timing.py [OUT.json]      (writes profiles/reward_stream_timing.json by default)"""
import json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, E, THRE, PICK_RATE = 1024, 5, 20, 0.5
STEP_LIMIT_S = 240
GRAM_MAX_WS = 8 * 2 ** 30
LEAN_FP32_TFLOPS = 117.0
RUNS = [("twitch_lol_8", [3600, 4114, 4628, 5142, 5657, 6171, 6685, 7200]), ("T16384", [16384]), ("T65536", [65536])]
BREAKDOWN = "T65536"
TAGS = {"prep_ms": 15, "norm_ms": 16, "pass_ms": 17, "rows_ms": 18, "join_ms": 19}      # SUMK_PROF_REWARD_STREAM_* (include/sumk.h), in launch order


def worker(spec):
    import ctypes as C
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from summarizer_amd import _lib, kernels
    dev = torch.device("cuda:0")
    lens, reps, warm = spec["lens"], spec["reps"], spec["warmup"]
    lib = _lib.load()
    n = sum(lens)
    g = torch.Generator().manual_seed(n)
    x = ((0.5 * 2.35 / D ** 0.5) * torch.randn(n, D, generator=g).abs()).to(dev)      # pool5-like non-negative features, distances O(1)
    acts = (torch.rand(E, n, generator=g) < PICK_RATE).float().to(dev)
    sb = kernels.SeqBatch.get(lens, dev)
    flop = sum(2 * T * T * D for T in lens)
    out = {"lens": lens, "D": D, "E": E, "temp_dist_thre": THRE, "pick_rate": PICK_RATE, "reps": reps, "warmup": warm, "gram_flop": flop,
           "expected_ms_at_117_tflops": flop / (LEAN_FP32_TFLOPS * 1e12) * 1e3,
           "expectation_note": "2 T^2 D FLOP at the rate measured on the band products; not measured on this kernel",
           "col_split_plan": kernels.dsn_reward_stream_plan(sb),
           "stream_workspace_bytes": int(kernels.dsn_reward_workspace_bytes(D, sb, E, "stream")),
           "gram_workspace_bytes": int(lib.sumk_dsn_reward_workspace_bytes(D, sb.n_seq, sb.off_host_p, E))}

    def timed(path):
        for _ in range(warm):
            r = kernels.dsn_reward(x, sb, acts, temp_dist_thre=THRE, path=path)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); r = kernels.dsn_reward(x, sb, acts, temp_dist_thre=THRE, path=path); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        assert bool(torch.isfinite(r).all()) and bool((r > 0).all())
        return float(np.median(ts)), [round(t, 3) for t in ts], r

    out["stream_ms"], out["stream_ms_all"], rs = timed("stream")
    out["stream_tflops"] = flop / out["stream_ms"] / 1e9
    if spec["name"] == BREAKDOWN:      # the launches, on calls of their own (not part of the timed calls above)
        lib.sumk_prof_enable(sum(1 << t for t in TAGS.values()))
        for t in TAGS.values():
            lib.sumk_prof_read(t, None, None, 1)
        for _ in range(reps):
            kernels.dsn_reward(x, sb, acts, temp_dist_thre=THRE, path="stream")
        torch.cuda.synchronize()
        for name, t in TAGS.items():
            ms, cnt = C.c_double(0.0), C.c_int64(0)
            lib.sumk_prof_read(t, C.byref(ms), C.byref(cnt), 1)
            out[name] = ms.value / max(cnt.value, 1)
        lib.sumk_prof_enable(0)
    if out["gram_workspace_bytes"] == 0 or out["gram_workspace_bytes"] > GRAM_MAX_WS:
        out["gram_skipped"] = (f"the Gram path asks for {out['gram_workspace_bytes']} bytes of workspace, past this script's cap of {GRAM_MAX_WS}: "
                               "not run, not estimated")
    else:
        out["gram_ms"], out["gram_ms_all"], rg = timed("gram")
        out["gram_over_stream"] = out["gram_ms"] / out["stream_ms"]
        out["stream_not_slower"] = out["stream_ms"] <= out["gram_ms"]
        out["max_abs_stream_minus_gram"] = float((rs - rg).abs().max())
    print("RESULT " + json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "reward_stream_timing.json")
    res = {"box": "1x MI355X", "D": D, "E": E, "precision": "fp32", "call": "kernels.dsn_reward, HIP events around one call", "runs": {}}
    for name, lens in RUNS:
        spec = {"name": name, "lens": lens, "reps": 5, "warmup": 2}
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(spec)], capture_output=True, text=True,
                               timeout=STEP_LIMIT_S, cwd=ROOT)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"{name}: no result within {STEP_LIMIT_S} s; nothing more was started"
            break
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res["stopped"] = f"{name}: exit code {r.returncode}; nothing more was started: {r.stderr[-600:]}"
            break
        res["runs"][name] = json.loads(line[-1][7:])
        print(f"{name}: " + line[-1][7:], flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(json.loads(sys.argv[2]))
    else:
        sys.exit(main())
