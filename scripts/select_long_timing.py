"""The long-video evaluation tail (sumk_eval_device_segments_long, sumk_eval_device_select_long; csrc/evallong.hip) beside the host tail
(sumk_eval_videos with the segment means given) and beside the one-workgroup kernel, on
  (a) a Twitch-LOL-shaped batch: 63 videos, T ~ U(3600, 7200) steps, 15 frames per step, 20 annotators, a segment per ~60 steps --
      segments and select under HIP events, the host tail once (wall clock);
  (b) one video of 65 536 steps x 15 frames = 983 040 frames, 1024 segments, a budget of 147 456 frames -- the new entries under HIP
      events (beside the 209 ms sumk_kts_banded takes in front of them, profiles/kts_banded_timing.json); the host tail once, in a child
      of its own that is given a minute: past it the record says "not run" and gives the operation count instead;
  (c) the worst case of profiles/select_timing.json, 1024 live segments at a budget of 8191, through sumk_eval_device_select and
      through sumk_eval_device_select_long: the ratio says where a default dispatch would switch (there is none yet).
Record, not a gate.  The measuring process is a child of this script and runs under a time limit, so a hang ends it:
    python scripts/select_long_timing.py [OUT.json]         (prints the JSON record and a README table row; writes the record to OUT.json,
                                                             default profiles/select_long_timing.json)"""
import ctypes as C
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420
HOST_B_LIMIT_S = 60


def _video_b(np):
    """(b): (means, nfps, n_frames, capacity) of the one long video, the same in the GPU worker and in the host child."""
    rng = np.random.default_rng(21)
    n_frames, S = 65536 * 15, 1024
    w = rng.multinomial(n_frames, np.ones(S) / S).astype(np.int32)
    return rng.random(S).astype(np.float32), w, n_frames, int(np.floor(n_frames * 0.15))


def _host_tail(np, _lib, vids):
    """sumk_eval_videos with seg_means given on (means, nfps, n_frames, mask or None) tuples -> (wall ms, frames selected, f_avg)."""
    lib, n = _lib.load(), len(vids)
    arr, keep, outs = (_lib.EvalVideo * n)(), [], []
    for e, (m, w, n_frames, mask) in zip(arr, vids):
        cps, out = np.zeros((len(m), 2), np.int32), np.empty(int(w.sum()), np.float32)
        keep.append(cps); outs.append(out)
        e.n_frames, e.n_steps, e.cps, e.nfps, e.n_segs, e.seg_means, e.machine_summary = n_frames, 1, cps.ctypes.data, w.ctypes.data, len(m), m.ctypes.data, out.ctypes.data
        if mask is not None:
            us = mask.astype(np.float32); keep.append(us)
            e.user_summary, e.n_users = us.ctypes.data, us.shape[0]
    t0 = time.perf_counter()
    _lib.check(lib.sumk_eval_videos(C.cast(arr, C.c_void_p), n, 0.15, 0, 0), "sumk_eval_videos")
    ms = (time.perf_counter() - t0) * 1e3
    return ms, sum(int(o.sum()) for o in outs), [arr[i].f_avg for i in range(n)]


def host_b():
    import numpy as np
    sys.path.insert(0, ROOT)
    from summarizer_amd import _lib
    m, w, n_frames, _ = _video_b(np)
    ms, frames, _ = _host_tail(np, _lib, [(m, w, n_frames, None)])
    print("HOST-B", json.dumps({"ms": ms, "frames_selected": frames}))


def worker(out_path):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native as N
    lib, dev = _lib.load(), torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rec = {"box": "1x MI355X", "date": time.strftime("%Y-%m-%d")}

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

    def select_setup(vids, entry):
        """Descriptors and buffers for (means, nfps, n_frames, mask) tuples -> (call, status, selected, f)."""
        n = len(vids)
        means = torch.from_numpy(np.concatenate([v[0] for v in vids])).to(dev)
        nfps = torch.from_numpy(np.concatenate([v[1] for v in vids])).to(dev)
        masks = [torch.from_numpy(v[3]).to(dev) if v[3] is not None else None for v in vids]
        d = (_lib.EvalDevSelect * n)()
        seg_at = at = 0
        for i, (m, w, n_frames, _) in enumerate(vids):
            d[i].seg_means, d[i].nfps, d[i].n_segs = means.data_ptr() + 4 * seg_at, nfps.data_ptr() + 4 * seg_at, len(m)
            d[i].n_frames, d[i].capacity, d[i].summary_len = n_frames, N.select_capacity(n_frames, 0.15), int(w.sum())
            d[i].summary0, d[i].sel0, d[i].method = at, seg_at, 0
            if masks[i] is not None:
                d[i].user_mask, d[i].n_users = masks[i].data_ptr(), masks[i].shape[0]
            seg_at += len(m); at += d[i].summary_len
        dd = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(dev)
        summary, selected = torch.empty(at, dtype=torch.float32, device=dev), torch.empty(seg_at, dtype=torch.uint8, device=dev)
        f, status = torch.empty(2 * n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        size_of, fn = ((lib.sumk_eval_device_select_long_workspace_bytes, lib.sumk_eval_device_select_long) if entry == "long" else
                       (lib.sumk_eval_device_select_workspace_bytes, lib.sumk_eval_device_select))
        ws = torch.empty(size_of(n, max(e.n_segs for e in d), max(e.capacity for e in d)), dtype=torch.uint8, device=dev)

        def call():
            _lib.check(fn(dd.data_ptr(), C.cast(d, C.c_void_p), n, summary.data_ptr(), at, selected.data_ptr(), seg_at, f.data_ptr(), f.data_ptr() + 8 * n,
                          status.data_ptr(), ws.data_ptr(), ws.numel(), st), "select")
        call.keep = (means, nfps, masks, dd, d, ws, summary)
        return call, status, selected, f, ws.numel()

    # ---- (a) the Twitch-LOL-shaped batch
    rng = np.random.default_rng(20)
    lens = [int(t) for t in rng.integers(3600, 7201, size=63)]
    vids, seg_descr, picks, cps_dev, scores = [], (_lib.EvalDevVideo * 63)(), [], [], torch.from_numpy(rng.random(sum(lens)).astype(np.float32)).to(dev)
    row0 = frame0 = seg0 = 0
    for i, T in enumerate(lens):
        n_frames, S = 15 * T, T // 60
        w = rng.multinomial(n_frames, np.ones(S) / S).astype(np.int32)
        hi = np.cumsum(w)
        vids.append((rng.random(S).astype(np.float32), w, n_frames, (rng.random((20, n_frames)) < 0.15).astype(np.uint8)))
        picks.append(torch.arange(0, n_frames, 15, dtype=torch.int32, device=dev))
        cps_dev.append(torch.from_numpy(np.stack([hi - w, hi - 1], axis=1).astype(np.int32)).to(dev))
        e = seg_descr[i]
        e.picks, e.n_picks, e.n_frames, e.n_steps, e.row0, e.frame0 = picks[i].data_ptr(), T, n_frames, T, row0, frame0
        e.cps, e.n_segs, e.seg0 = cps_dev[i].data_ptr(), S, seg0
        row0 += T; frame0 += n_frames; seg0 += S
    seg_dd = torch.frombuffer(bytearray(bytes(seg_descr)), dtype=torch.uint8).to(dev)
    scratch, seg = torch.empty(frame0, dtype=torch.float32, device=dev), torch.empty(seg0, dtype=torch.float32, device=dev)
    seg_ms = events_ms(lambda: _lib.check(lib.sumk_eval_device_segments_long(scores.data_ptr(), seg_dd.data_ptr(), C.cast(seg_descr, C.c_void_p), 63,
                                                                            scratch.data_ptr(), seg.data_ptr(), st), "segments_long"), 10)
    call, status, selected, f, ws_bytes = select_setup(vids, "long")
    sel_ms = events_ms(call, 10)
    assert int(status.abs().sum()) == 0
    host_ms, _, host_f = _host_tail(np, _lib, vids)
    assert f.cpu().numpy()[:63].tolist() == host_f                       # the same F-scores, bit for bit
    rec["a_twitch_lol_shape"] = {"videos": 63, "steps": sum(lens), "frames": frame0, "segments": seg0, "annotators": 20,
                                 "largest_budget": max(N.select_capacity(v[2], 0.15) for v in vids), "segments_long_ms": seg_ms, "select_long_ms": sel_ms,
                                 "select_workspace_bytes": ws_bytes, "segments_selected": int(selected.sum()), "host_tail_wall_ms_one_call": host_ms}
    del call, vids

    # ---- (b) one video of 65 536 steps
    m, w, n_frames, cap = _video_b(np)
    hi = np.cumsum(w)
    pk = torch.arange(0, n_frames, 15, dtype=torch.int32, device=dev)
    cp = torch.from_numpy(np.stack([hi - w, hi - 1], axis=1).astype(np.int32)).to(dev)
    sc = torch.from_numpy(rng.random(65536).astype(np.float32)).to(dev)
    d1 = (_lib.EvalDevVideo * 1)()
    d1[0].picks, d1[0].n_picks, d1[0].n_frames, d1[0].n_steps, d1[0].cps, d1[0].n_segs = pk.data_ptr(), 65536, n_frames, 65536, cp.data_ptr(), 1024
    d1d = torch.frombuffer(bytearray(bytes(d1)), dtype=torch.uint8).to(dev)
    scratch, seg = torch.empty(n_frames, dtype=torch.float32, device=dev), torch.empty(1024, dtype=torch.float32, device=dev)
    seg_ms = events_ms(lambda: _lib.check(lib.sumk_eval_device_segments_long(sc.data_ptr(), d1d.data_ptr(), C.cast(d1, C.c_void_p), 1, scratch.data_ptr(),
                                                                            seg.data_ptr(), st), "segments_long"), 10)
    call, status, selected, f, ws_bytes = select_setup([(m, w, n_frames, None)], "long")
    sel_ms = events_ms(call, 5)
    assert int(status.abs().sum()) == 0
    picked = int(selected.sum())
    b = {"steps": 65536, "frames": n_frames, "segments": 1024, "budget": cap, "segments_long_ms": seg_ms, "select_long_ms": sel_ms,
         "select_workspace_bytes": ws_bytes, "segments_selected": picked, "frames_selected": int((selected.cpu().numpy() * w).sum()),
         "kts_banded_ms_in_front": 209, "host_tail_operations": int(1024 * (cap + 1) * (picked + 1))}
    try:      # the host tail in a child of its own, given a minute (it opens no GPU)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "host_b"], timeout=HOST_B_LIMIT_S, capture_output=True, text=True).stdout
        hb = json.loads(out.split("HOST-B", 1)[1])
        assert hb["frames_selected"] == b["frames_selected"]
        b["host_tail_wall_ms_one_call"] = hb["ms"]
    except subprocess.TimeoutExpired:
        b["host_tail_wall_ms_one_call"] = f"not run: over {HOST_B_LIMIT_S} s"
    rec["b_one_video_65536_steps"] = b
    del call

    # ---- (c) 1024 live segments at a budget of 8191, both entries
    rng = np.random.default_rng(3)
    cap, S, n_frames = 8191, 1024, 54607
    assert N.select_capacity(n_frames, 0.15) == cap
    m = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), size=S)
    w = rng.integers(cap // 40, cap // 10, size=S).astype(np.int32)
    c = {}
    for entry in ("block", "long"):
        call, status, selected, f, _ = select_setup([(m, w, n_frames, None)], entry)
        c[f"{entry}_ms"] = events_ms(call, 10)
        assert int(status.abs().sum()) == 0
        c[f"{entry}_segments_selected"] = int(selected.sum())
    assert c["block_segments_selected"] == c["long_segments_selected"]
    c["long_over_block"] = c["long_ms"] / c["block_ms"]
    rec["c_one_video_1024_segments_budget_8191"] = c

    line = json.dumps(rec)
    print("SELECT-LONG-TIMING", line)
    a = rec["a_twitch_lol_shape"]
    host_b_txt = f"{b['host_tail_wall_ms_one_call'] / 1e3:.1f} s" if not isinstance(b["host_tail_wall_ms_one_call"], str) else \
        f"{b['host_tail_wall_ms_one_call']} ({b['host_tail_operations']:.2e} table entries)"
    print("README-ROW",
          f"Measured (1x MI355X, {rec['date']}, `profiles/select_long_timing.json`, HIP events): 63 videos of 3600 .. 7200 steps x 15 frames, 20 annotators "
          f"(Twitch-LOL shape): segments {a['segments_long_ms']:.2f} ms + select {a['select_long_ms']:.2f} ms against {a['host_tail_wall_ms_one_call']:.0f} ms for the host "
          f"tail (one call); one video of 65 536 steps, 1024 segments, budget 147 456: segments {b['segments_long_ms']:.2f} ms + select {b['select_long_ms']:.1f} ms "
          f"behind the 209 ms of `sumk_kts_banded`, host tail {host_b_txt}; 1024 live segments at budget 8191: {c['long_ms']:.2f} ms against {c['block_ms']:.2f} ms for "
          f"`sumk_eval_device_select` ({c['long_over_block']:.1f}x)")
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "host_b":
        host_b()
    else:
        out = ([a for a in sys.argv[1:] if a.endswith(".json")] or [os.path.join(ROOT, "profiles", "select_long_timing.json")])[0]
        # a fresh child does the GPU work (this process never opens the device) under a time limit of its own
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "worker", out], timeout=LIMIT_S).returncode)
