"""Inter-annotator agreement on the device (summarizer_amd/utils/agreement.py, csrc/agreement.hip) beside the host specification, on the
50-video S-TVSum shape (recipes.synthetic_video geometry: 150 .. 320 steps, a pick every 15 frames; 20 annotators grading 1 .. 5 over
two-second blocks and marking key shots over one-second blocks), for both correlation metrics:
  (a) ONE `human_agreement` call end to end (host checks, the one upload, the enqueued chain, the one D2H): host wall clock;
  (b) the enqueued chain alone -- sumk_rank_rows, sumk_agreement_corr, sumk_agreement_f -- under HIP events on fixed buffers (Kendall: also
      with every pair through the LDS sort instead of the contingency tables these graded rows qualify for);
  (c) the same numbers from the host specification (tests/agreement_ref.py: numpy + scipy) in the same process, wall clock, one call.
(a) and (b): the median, the extremes and the quartiles of 30 timed calls after 3 warm-up calls.  The results of (a) are held to (c)
before anything is reported.  The measuring process is a child of this script and runs under a time limit, so a hang ends it:
    python scripts/agreement_timing.py [OUT.json]            (prints the JSON record; writes it to OUT.json, default profiles/agreement_timing.json)"""
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420


def worker(out_path):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import annotate_ref as A
    import agreement_ref as S
    import recipes as R
    from summarizer_amd.utils import agreement as M
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    lens = [int(t) for t in rng.integers(150, 321, size=50)]
    videos = {}
    for i, T in enumerate(lens):
        nf = int(R.synthetic_video(T, 9100 + i, n_users=20)["n_frames"])
        videos[f"video_{i + 1}"] = {"user_scores": ((A.block_grades(20, nf, 9200 + i, block=60) - np.float32(1)) / np.float32(4)).astype(np.float32),
                                    "user_summary": A.block_selections(20, nf, 9300 + i, block=30)}
    frames = sum(v["user_scores"].shape[1] for v in videos.values())
    rec = {"box": "1x " + torch.cuda.get_device_name(dev), "date": time.strftime("%Y-%m-%d"), "videos": 50, "annotators": 20, "frames": frames,
           "pairs_per_video": 190, "input_bytes": 2 * 4 * 20 * frames}

    def stats(ts):
        q = np.percentile(ts, [25, 75])
        return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "q25": float(q[0]), "q75": float(q[1]), "calls": len(ts)}

    def wall_ms(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, out
    def chain_ms(chain):
        for _ in range(3):
            chain.enqueue()
        torch.cuda.synchronize()
        ev = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); chain.enqueue(); e1.record(); e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        return ev
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    summ, sc = [up(v["user_summary"]) for v in videos.values()], [up(v["user_scores"]) for v in videos.values()]
    for metric in ("spearmanr", "kendalltau"):
        wall_ms(lambda: M.human_agreement(videos, metric), 3)        # warm the kernels and the allocator
        ts, got = wall_ms(lambda: M.human_agreement(videos, metric), 30)
        rec[f"a_human_agreement_wall_ms/{metric}"] = stats(ts)
        chain = M.AgreementChain(summ, sc, metric)
        rec[f"b_chain_hip_events_ms/{metric}"] = stats(chain_ms(chain))
        if metric == "kendalltau":                                   # the same chain with every pair through the LDS sort (no contingency tables)
            rec["b_chain_sort_only_hip_events_ms/kendalltau"] = stats(chain_ms(M.AgreementChain(summ, sc, metric, _sort_only=True)))
        rec["b_rank_scratch_bytes"] = int(chain.scratch.numel())
        ts, want = wall_ms(lambda: {k: S.agreement(v["user_summary"], v["user_scores"], metric) for k, v in videos.items()}, 1)
        rec[f"c_host_specification_wall_ms/{metric}"] = stats(ts)
        same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
        for k in videos:
            for f in ("F", "C", "f_avg_user", "f_max_user", "corr_user", "f_avg", "f_max", "corr"):
                assert same(got["videos"][k][f], want[k][f]), (metric, k, f)
        rec[f"human_row/{metric}"] = {"corr": got["corr"], "f_avg": got["f_avg"], "f_max": got["f_max"]}
    rec["results_equal_specification"] = True
    line = json.dumps(rec)
    print("AGREEMENT-TIMING", line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        out = [a for a in sys.argv[1:] if a.endswith(".json")][:1] or [os.path.join(ROOT, "profiles", "agreement_timing.json")]
        # a fresh child does the GPU work (this process never opens the device) under a time limit of its own
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "worker"] + out, timeout=LIMIT_S).returncode)
