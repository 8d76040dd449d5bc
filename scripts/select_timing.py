"""Key-shot selection on the device (sumk_eval_device_select, csrc/evalselect.hip) beside the host tail, on
  (a) the 50-video S-TVSum batch shape (recipes.synthetic_video, 150 .. 320 steps, 15 annotators): ONE `evaluate_batch_device` call end to
      end with select="host" (the baseline: the code as it was before the device path) and with select="device", in the same process --
      the host wall clock around the call, median of repeated calls, in both orders;
  (b) the select launch alone on that batch under HIP events;
  (c) one worst-case video -- 1024 live segments, budget 8191 -- i.e. what one workgroup's 1024 dependent barrier steps over workspace
      rows cost, and the same video at budget 4095 (rows in LDS).
The measuring process is a child of this script and runs under a time limit, so a hang ends it:
    python scripts/select_timing.py [OUT.json]              (prints the JSON record, and writes it to OUT.json when given)"""
import ctypes as C
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300


def worker(out_path):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import recipes as R
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native as N
    lib, dev = _lib.load(), torch.device("cuda:0")
    rng = np.random.default_rng(3)
    lens = [int(t) for t in rng.integers(150, 321, size=50)]
    vids = []
    for i, T in enumerate(lens):
        v = R.synthetic_video(T, 9100 + i, n_users=15)
        vids.append(N.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"], E.rank_users(v["user_scores"])))
    scores = torch.from_numpy(rng.random(sum(lens)).astype(np.float32)).to(dev)
    rec = {"box": "1x MI355X", "date": time.strftime("%Y-%m-%d"), "videos": 50, "steps": sum(lens), "frames": sum(v["n_frames"] for v in vids),
           "segments": sum(v["cps"].shape[0] for v in vids), "largest_budget": max(N.select_capacity(v["n_frames"], 0.15) for v in vids)}

    def wall_ms(select, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = N.evaluate_batch_device(vids, scores, lens, 0.15, "knapsack", select=select)
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, out
    for select in N.SELECTS:                                   # build the caches, warm the kernels
        wall_ms(select, 3)
    a = {}
    for order in (("host", "device"), ("device", "host")):
        for select in order:
            ts, out = wall_ms(select, 30)
            a.setdefault(select, []).extend(ts)
            a[select + "_f_avg_mean"] = float(np.mean(out[1]))
    assert a["host_f_avg_mean"] == a["device_f_avg_mean"]
    rec["a_evaluate_batch_device_wall_ms"] = {k: {"median": float(np.median(a[k])), "min": float(np.min(a[k])), "calls": len(a[k])} for k in N.SELECTS}

    def launch_ms(descr, n, summary_total, seg_total, reps):
        """HIP events around sumk_eval_device_select alone: descriptors (ctypes array) -> median ms."""
        dd = torch.frombuffer(bytearray(bytes(descr)), dtype=torch.uint8).to(dev)
        summary = torch.empty(max(summary_total, 1), dtype=torch.float32, device=dev)
        selected = torch.empty(seg_total, dtype=torch.uint8, device=dev)
        f, status = torch.empty(2 * n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.sumk_eval_device_select_workspace_bytes(n, max(d.n_segs for d in descr), max(d.capacity for d in descr)), dtype=torch.uint8, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def call():
            _lib.check(lib.sumk_eval_device_select(dd.data_ptr(), C.cast(descr, C.c_void_p), n, summary.data_ptr(), summary_total, selected.data_ptr(),
                                                   seg_total, f.data_ptr(), f.data_ptr() + 8 * n, status.data_ptr(), ws.data_ptr(), ws.numel(), st), "select")
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        assert int(status.abs().sum()) == 0
        return float(np.median(ts)), int(selected.sum())
    # (b) the same 50 videos through the C entry, on descriptors and buffers of this script's own (segment means drawn like the scores)
    n_seg = [v["cps"].shape[0] for v in vids]
    means = torch.from_numpy(rng.random(sum(n_seg)).astype(np.float32)).to(dev)
    nfps_dev = torch.from_numpy(np.concatenate([v["nfps"] for v in vids])).to(dev)
    masks = [torch.from_numpy((v["user_summary"] > 0).astype(np.uint8)).to(dev) for v in vids]
    d = (_lib.EvalDevSelect * 50)()
    seg_at = at = 0
    for i, v in enumerate(vids):
        d[i].seg_means, d[i].nfps, d[i].n_segs = means.data_ptr() + 4 * seg_at, nfps_dev.data_ptr() + 4 * seg_at, n_seg[i]
        d[i].n_frames, d[i].capacity, d[i].summary_len = v["n_frames"], N.select_capacity(v["n_frames"], 0.15), int(v["nfps"].sum())
        d[i].summary0, d[i].sel0, d[i].user_mask, d[i].n_users, d[i].method = at, seg_at, masks[i].data_ptr(), masks[i].shape[0], 0
        seg_at += n_seg[i]; at += d[i].summary_len
    ms, picked = launch_ms(d, 50, at, seg_at, 30)
    rec["b_select_launch_ms"] = {"median": ms, "segments_selected": picked}
    # (c) one video, 1024 live segments (positive values, weights that fit), budget 8191 / 4095
    for cap in (8191, 4095):
        S = 1024
        means = torch.from_numpy(rng.choice(np.array([0.25, 0.5, 0.75], np.float32), size=S)).to(dev)
        w = rng.integers(cap // 40, cap // 10, size=S).astype(np.int32)
        nfps = torch.from_numpy(w).to(dev)
        d = (_lib.EvalDevSelect * 1)()
        d[0].seg_means, d[0].nfps, d[0].n_segs, d[0].n_frames, d[0].capacity = means.data_ptr(), nfps.data_ptr(), S, cap, cap
        d[0].summary_len, d[0].summary0, d[0].sel0, d[0].method = int(w.sum()), 0, 0, 0
        ms, picked = launch_ms(d, 1, int(w.sum()), S, 10)
        rec[f"c_one_video_1024_segments_budget_{cap}_ms"] = {"median": ms, "segments_selected": picked,
                                                             "rows": "workspace" if cap > N.SELECT_LDS_CAPACITY else "LDS"}
    line = json.dumps(rec)
    print("SELECT-TIMING", line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        out = [a for a in sys.argv[1:] if a.endswith(".json")][:1]
        # a fresh child does the GPU work (this process never opens the device) under a time limit of its own
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "worker"] + out, timeout=LIMIT_S).returncode)
