"""The long-video rank correlation (sumk_eval_device_spearman_long, sumk_eval_device_kendall_long; csrc/evalcorr_long.hip) beside the host
tail on the same input (sumk_eval_videos / sumk_eval_videos_kendall through utils.eval_native.evaluate_batch, one call, wall clock) and
beside the one-workgroup kernels, on
  (a) the Twitch-LOL-shaped batch of scripts/select_long_timing.py: 63 videos, T ~ U(3600, 7200) steps, 15 frames per step, 20 annotators;
  (b) one video of 65 536 steps x 15 frames = 983 040 frames, 20 annotators;
  (c) the S-TVSum shape: 50 videos, T ~ U(150, 320) steps, 15 frames per step, 20 annotators -- through the block kernels
      (sumk_eval_device_spearman / sumk_eval_device_kendall) and through the long ones: the ratio says where a dispatch would switch
      (there is none).
Both metrics; device chains under HIP events (median).  Annotators grade on five levels per 30-frame shot (TVSum style).  Record, not a
gate.  The measuring process is a child of this script and runs under a time limit, so a hang ends it:
    python scripts/corr_long_timing.py [OUT.json] [only=a|b|c]    (prints the JSON record and a README row; writes the record to OUT.json,
                                                                   default profiles/corr_long_timing.json)"""
import ctypes as C
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 540


def worker(out_path, only):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native as N
    lib, dev = _lib.load(), torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rec = {"box": "1x MI355X", "date": time.strftime("%Y-%m-%d"), "tile": N.CORR_LONG_TILE}

    def events_ms(call, reps):
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    def videos(lens, seed, n_users=20):
        rng = np.random.default_rng(seed)
        out = []
        for T in lens:
            n_frames = 15 * T
            grades = rng.integers(1, 6, size=(n_users, n_frames // 30 + 1)).repeat(30, axis=1)[:, :n_frames].astype(np.float32)
            v = N.prepare_video(n_frames, np.arange(0, n_frames, 15), user_ranks=E.rank_users(grades))
            out.append((v, rng.random(T).astype(np.float32)))
        return out

    def measure(vs, reps, block=False):
        """Both metrics on (video, scores) pairs -> record.  The device results are checked against the host's before a time is kept."""
        n = len(vs)
        scores = torch.from_numpy(np.concatenate([s for _, s in vs])).to(dev)
        d, kd, keep = (_lib.EvalDevVideo * n)(), (_lib.EvalDevKendall * n)(), []
        row0 = frame0 = users = 0
        for i, (v, s) in enumerate(vs):
            ru = v["user_ranks"]
            mu = ru.sum(axis=1) / ru.shape[1]
            dense, ytie = N._kendall_meta(v)
            t = [torch.from_numpy(a).to(dev) for a in (v["picks"], ru, mu, ((ru - mu[:, None]) ** 2).sum(axis=1), dense, ytie)]
            keep.append(t)
            d[i].picks, d[i].n_picks, d[i].n_frames, d[i].n_steps, d[i].row0, d[i].frame0 = t[0].data_ptr(), len(v["picks"]), v["n_frames"], len(s), row0, frame0
            d[i].user_ranks, d[i].user_mean, d[i].user_ssq, d[i].n_users = t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), ru.shape[0]
            kd[i].y_dense, kd[i].ytie, kd[i].counts0 = t[4].data_ptr(), t[5].data_ptr(), users
            row0 += len(s); frame0 += v["n_frames"]; users += ru.shape[0]
        dd = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(dev)
        kdd = torch.frombuffer(bytearray(bytes(kd)), dtype=torch.uint8).to(dev)
        host = C.cast(d, C.c_void_p)
        corr, counts = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(4 * users, dtype=torch.int64, device=dev)
        r = {"videos": n, "steps": row0, "frames": frame0, "annotators": users // n}
        for metric in N.METRICS:
            kendall = metric == "kendalltau"
            nbytes = (lib.sumk_eval_device_kendall_long_workspace_bytes if kendall else lib.sumk_eval_device_spearman_long_workspace_bytes)(host, n)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            if kendall:
                def long_call():
                    _lib.check(lib.sumk_eval_device_kendall_long(scores.data_ptr(), dd.data_ptr(), host, kdd.data_ptr(), n, ws.data_ptr(), nbytes, corr.data_ptr(),
                                                                 counts.data_ptr(), st), "kendall_long")
            else:
                def long_call():
                    _lib.check(lib.sumk_eval_device_spearman_long(scores.data_ptr(), dd.data_ptr(), host, n, ws.data_ptr(), nbytes, corr.data_ptr(), st), "spearman_long")
            ms = events_ms(long_call, reps)
            got = corr.cpu().numpy().copy()
            t0 = time.perf_counter()
            want = N.evaluate_batch([v for v, _ in vs], [s for _, s in vs], metric=metric)[0]
            host_ms = (time.perf_counter() - t0) * 1e3
            if kendall:
                assert np.array_equal(got, want)                               # the same tau, bit for bit
            else:
                assert np.abs(got - want).max() <= 1e-12
            m = {"long_ms": ms, "workspace_bytes": int(nbytes), "host_tail_wall_ms_one_call": host_ms, "host_over_long": host_ms / ms}
            if block:
                if kendall:
                    scr = torch.empty(lib.sumk_eval_device_kendall_scratch_bytes(n, frame0), dtype=torch.uint8, device=dev)
                    m["block_ms"] = events_ms(lambda: _lib.check(lib.sumk_eval_device_kendall(scores.data_ptr(), dd.data_ptr(), kdd.data_ptr(), n, scr.data_ptr(),
                                                                                             corr.data_ptr(), counts.data_ptr(), st), "kendall"), reps)
                    assert np.array_equal(corr.cpu().numpy(), want)
                else:
                    scr = torch.empty(lib.sumk_eval_device_spearman_scratch_bytes(n), dtype=torch.uint8, device=dev)
                    m["block_ms"] = events_ms(lambda: _lib.check(lib.sumk_eval_device_spearman(scores.data_ptr(), dd.data_ptr(), n, scr.data_ptr(), corr.data_ptr(), st),
                                                                 "spearman"), reps)
                m["long_over_block"] = ms / m["block_ms"]
            r[metric] = m
            del ws
        return r

    if only in (None, "a"):
        rng = np.random.default_rng(20)
        rec["a_twitch_lol_shape"] = measure(videos([int(t) for t in rng.integers(3600, 7201, size=63)], 21), 5)
    if only in (None, "b"):
        rec["b_one_video_65536_steps"] = measure(videos([65536], 22), 5)
    if only in (None, "c"):
        rng = np.random.default_rng(23)
        rec["c_s_tvsum_shape"] = measure(videos([int(t) for t in rng.integers(150, 321, size=50)], 24), 10, block=True)
    line = json.dumps(rec)
    print("CORR-LONG-TIMING", line)
    if only is None:
        a, b, c = rec["a_twitch_lol_shape"], rec["b_one_video_65536_steps"], rec["c_s_tvsum_shape"]

        def pair(r, m):
            return f"{r[m]['long_ms']:.2f} ms against {r[m]['host_tail_wall_ms_one_call']:.0f} ms for the host tail ({r[m]['host_over_long']:.0f}x)"
        print("README-ROW",
              f"Measured (1x MI355X, {rec['date']}, `profiles/corr_long_timing.json`, HIP events): 63 videos of 3600 .. 7200 steps x 15 frames, 20 annotators "
              f"(Twitch-LOL shape): Spearman {pair(a, 'spearmanr')}, Kendall {pair(a, 'kendalltau')}; one video of 65 536 steps, 983 040 frames, 20 annotators: "
              f"Spearman {pair(b, 'spearmanr')}, Kendall {pair(b, 'kendalltau')}; 50 videos of the S-TVSum shape: Spearman {c['spearmanr']['long_ms']:.2f} ms against "
              f"{c['spearmanr']['block_ms']:.2f} ms for `sumk_eval_device_spearman` ({c['spearmanr']['long_over_block']:.1f}x), Kendall "
              f"{c['kendalltau']['long_ms']:.2f} ms against {c['kendalltau']['block_ms']:.2f} ms for `sumk_eval_device_kendall` ({c['kendalltau']['long_over_block']:.1f}x)")
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    only = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("only=")] or [None])[0]
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(sys.argv[2], only)
    else:
        out = ([a for a in sys.argv[1:] if a.endswith(".json")] or [os.path.join(ROOT, "profiles", "corr_long_timing.json")])[0]
        # a fresh child does the GPU work (this process never opens the device) under a time limit of its own
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "worker", out] + ([f"only={only}"] if only else []), timeout=LIMIT_S).returncode)
