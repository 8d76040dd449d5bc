"""Dataset records from raw annotations on the device (summarizer_amd/utils/annotate.py, csrc/annotate.hip) beside the host specification, on
the 50-video S-TVSum shape (recipes.synthetic_video geometry: 150 .. 320 steps, a pick every 15 frames, 20 annotators grading 1 .. 5 over
two-second blocks, the videos' own change points):
  (a) ONE `build_records` call end to end (host checks, uploads, the enqueued chain, the one D2H, the records): host wall clock, median;
  (b) the enqueued chain alone -- sumk_annotate, sumk_eval_device_segments, sumk_eval_device_select with 21 problems per video,
      sumk_annotate_gtsummary -- under HIP events on fixed buffers, median;
  (c) the same records from the host specification (tests/annotate_ref.py: numpy + the native host knapsack) in the same process, wall clock.
The records of (a) are held to (c) field by field before anything is reported.  The measuring process is a child of this script and runs
under a time limit, so a hang ends it:
    python scripts/annotate_timing.py [OUT.json]            (prints the JSON record; writes it to OUT.json, default profiles/annotate_timing.json)"""
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300


def worker(out_path):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import annotate_ref as A
    import recipes as R
    from summarizer_amd.utils import annotate as M
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    lens = [int(t) for t in rng.integers(150, 321, size=50)]
    videos = {}
    for i, T in enumerate(lens):
        v = R.synthetic_video(T, 9100 + i, n_users=20)
        videos[f"video_{i + 1}"] = {"features": np.zeros((T, 4), np.float32), "picks": v["picks"], "n_frames": v["n_frames"],
                                    "change_points": v["change_points"], "n_frame_per_seg": v["n_frame_per_seg"],
                                    "annotations": A.block_grades(20, v["n_frames"], 9200 + i, block=60)}
    frames = sum(v["n_frames"] for v in videos.values())
    rec = {"box": "1x " + torch.cuda.get_device_name(dev), "date": time.strftime("%Y-%m-%d"), "videos": 50, "annotators": 20, "steps": sum(lens), "frames": frames,
           "segments": sum(len(v["n_frame_per_seg"]) for v in videos.values()), "selection_problems": 50 * 21,
           "annotation_bytes": 4 * 20 * frames}

    def wall_ms(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, out
    wall_ms(lambda: M.build_records(videos), 3)                   # warm the kernels and the allocator
    ts, ds = wall_ms(lambda: M.build_records(videos), 20)
    rec["a_build_records_wall_ms"] = {"median": float(np.median(ts)), "min": float(np.min(ts)), "calls": len(ts)}
    # (b) the chain alone, on fixed buffers
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vs = list(videos.values())
    chain = M.AnnotateChain([up(v["annotations"]) for v in vs], [up(v["picks"]) for v in vs], [v["n_frames"] for v in vs],
                            [(up(v["change_points"]), up(v["n_frame_per_seg"])) for v in vs])
    for _ in range(3):
        chain.enqueue()
    torch.cuda.synchronize()
    ev = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); chain.enqueue(); e1.record(); e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    rec["b_chain_hip_events_ms"] = {"median": float(np.median(ev)), "min": float(np.min(ev)), "calls": len(ev)}
    rec["b_select_workspace_bytes"] = int(chain.ws.numel())
    # (c) the host specification, same process
    def host():
        return {k: A.record(v["annotations"], v["picks"], v["n_frames"], v["change_points"], v["n_frame_per_seg"]) for k, v in videos.items()}
    ts, want = wall_ms(host, 3)
    rec["c_host_specification_wall_ms"] = {"median": float(np.median(ts)), "min": float(np.min(ts)), "calls": len(ts)}
    for k in videos:
        for f in ("user_scores", "user_summary", "gtscore", "gtsummary"):
            assert np.array_equal(ds[k][f][...], want[k][f]), (k, f)
    rec["records_equal_specification"] = True
    rec["frames_in_user_summaries"] = int(sum(ds[k]["user_summary"][...].sum() for k in videos))
    line = json.dumps(rec)
    print("ANNOTATE-TIMING", line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        out = [a for a in sys.argv[1:] if a.endswith(".json")][:1] or [os.path.join(ROOT, "profiles", "annotate_timing.json")]
        # a fresh child does the GPU work (this process never opens the device) under a time limit of its own
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "worker"] + out, timeout=LIMIT_S).returncode)
