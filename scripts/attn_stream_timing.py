"""The Transformer scorer with attention="stream" (csrc/attn_stream.hip: no (T x T) logits) beside the dense path on long videos.

D = 1024, 8 heads of 128 columns, F = D, 6 layers, exact fp32, one video (and the 50-video S-TVSum shape, T ~ U(150, 320)):
  * T = 4096, 8192: the attention of one layer both ways -- the stream launch against the dense core's three launches (logits, softmax,
    context), event pairs of the library's profiler around each inside the same 6-layer scoring calls -- and the whole score_packed both ways;
  * T = 16384, 65536: the stream path alone.  The dense run is skipped there -- its workspace query answers more than DENSE_MAX_WS (about
    8.6 GB and 137 GB) -- and the record says so with the bytes it asked for: not run, not estimated;
  * the S-TVSum batch: both ways (the dense path is expected to stay the better choice at these lengths; recorded either way);
  * the attention launch alone at head width 256 (D = 2048, 8 heads, T = 8192): the instance that spills registers, so that its rate is on record.
Expectation, recorded beside each measurement: 4 T^2 D FLOP per layer at the rate the lean fp32 MFMA kernel reaches in the band products
(about 117 TFLOP/s, README) -- 0.6 / 2.35 / 9.4 / 150 ms at T = 4096 / 8192 / 16384 / 65536.  That rate was measured on the band products,
not on this kernel, whose first product contracts only 128 columns per tile.  The one condition: at T = 8192 the stream attention launch is
not slower than the dense core's three launches in the same run ("stream_attention_not_slower").
Per run: the median over 5 calls of one call's stream time (HIP events around the call, 2 warm-up calls first); per-launch figures are
the profiler's mean over those calls' launches.  Every GPU step is a fresh child of this script under its own time limit; after a step
that fails or runs out of time nothing more is started.
    python scripts/attn_stream_timing.py [OUT.json]      (writes profiles/attn_stream_timing.json by default)"""
import json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HEADS, LAYERS = 1024, 8, 6
STEP_LIMIT_S = 240
DENSE_MAX_WS = 8 * 2 ** 30
LEAN_FP32_TFLOPS = 117.0


def runs():
    import numpy as np
    tvsum = [int(t) for t in np.random.default_rng(11).integers(150, 321, size=50)]
    return [("T4096", [4096]), ("T8192", [8192]), ("T16384", [16384]), ("T65536", [65536]), ("s_tvsum_50", tvsum),
            ("T8192_dh256_attention_only", [8192])]


def attention_only(spec, lib, kernels, tag):
    """kernels.attn_stream by itself on one video at another head width (dh = 256: the D = 2048 stacks): the launch under the profiler."""
    import ctypes as C
    import torch
    dev = torch.device("cuda:0")
    T, Dm, heads, reps, warm = spec["lens"][0], spec["D"], spec["heads"], spec["reps"], spec["warmup"]
    g = torch.Generator().manual_seed(T)
    q, k, v = ((0.5 * torch.randn(T, Dm, generator=g)).to(dev) for _ in range(3))
    sb = kernels.SeqBatch.get([T], dev)
    for _ in range(warm):
        out = kernels.attn_stream(q, k, v, sb, heads)
    torch.cuda.synchronize()
    lib.sumk_prof_enable(1 << tag)
    lib.sumk_prof_read(tag, None, None, 1)
    for _ in range(reps):
        out = kernels.attn_stream(q, k, v, sb, heads)
    torch.cuda.synchronize()
    ms, cnt = C.c_double(0.0), C.c_int64(0)
    lib.sumk_prof_read(tag, C.byref(ms), C.byref(cnt), 1)
    lib.sumk_prof_enable(0)
    assert cnt.value == reps and bool(torch.isfinite(out).all())
    flop = 4 * T * T * Dm
    res = {"lens": [T], "D": Dm, "heads": heads, "head_width": Dm // heads, "reps": reps, "warmup": warm, "attention_flop": flop,
           "stream_attention_ms": ms.value / reps, "stream_attention_tflops": flop / (ms.value / reps) / 1e9,
           "note": "kernels.attn_stream alone; this instance spills registers (csrc/attn_stream.hip header) and is not tuned"}
    print("RESULT " + json.dumps(res))


def worker(spec):
    import ctypes as C
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from summarizer_amd import _lib, kernels
    from summarizer_amd.models.transformer import Transformer
    dev = torch.device("cuda:0")
    lens, reps, warm = spec["lens"], spec["reps"], spec["warmup"]
    lib = _lib.load()
    TAG_DENSE, TAG_STREAM = _lib.PROF_TF_ATTN_DENSE, _lib.PROF_ATTN_STREAM      # SUMK_PROF_* of include/sumk.h
    if spec.get("attention_only"):
        return attention_only(spec, lib, kernels, TAG_STREAM)
    n = sum(lens)
    torch.manual_seed(n)
    models = {}
    for att in ("stream", "dense"):
        torch.manual_seed(7)
        models[att] = Transformer(input_size=D, encoder_layers=LAYERS, attention_heads=HEADS, attention=att).to(dev).eval()
    models["dense"].load_state_dict(models["stream"].state_dict())
    x = (0.5 * torch.randn(n, D, generator=torch.Generator().manual_seed(n))).to(dev)
    sb = kernels.SeqBatch.get(lens, dev)
    flop = sum(4 * T * T * D for T in lens)
    out = {"lens": lens if len(lens) < 8 else f"{len(lens)} videos, {n} steps", "D": D, "heads": HEADS, "layers": LAYERS, "reps": reps, "warmup": warm,
           "attention_flop_per_layer": flop, "expected_attention_ms_at_117_tflops": flop / (LEAN_FP32_TFLOPS * 1e12) * 1e3,
           "expectation_note": "4 T^2 D FLOP at the rate measured on the band products; not measured on this kernel",
           "stream_workspace_bytes": int(kernels.transformer_workspace_bytes(D, D, HEADS, LAYERS, sb, "stream")),
           "dense_workspace_bytes": int(lib.sumk_transformer_workspace_bytes(D, D, HEADS, LAYERS, sb.n_seq, sb.off_host_p, 0))}

    def timed(att, tag):
        m = models[att]
        with torch.no_grad():
            for _ in range(warm):
                s = m.score_packed(x, lens)
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); s = m.score_packed(x, lens); b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            assert bool(torch.isfinite(s).all())
            # the attention launches, on calls of their own (not part of the timed calls above)
            lib.sumk_prof_enable(1 << tag)
            lib.sumk_prof_read(tag, None, None, 1)
            for _ in range(reps):
                m.score_packed(x, lens)
            torch.cuda.synchronize()
            ms, cnt = C.c_double(0.0), C.c_int64(0)
            lib.sumk_prof_read(tag, C.byref(ms), C.byref(cnt), 1)
            lib.sumk_prof_enable(0)
        assert cnt.value == reps * LAYERS, (cnt.value, reps, LAYERS)
        return float(np.median(ts)), [round(t, 3) for t in ts], ms.value / cnt.value, s

    out["stream_score_ms"], out["stream_score_ms_all"], out["stream_attention_ms"], ss = timed("stream", TAG_STREAM)
    out["stream_attention_tflops"] = flop / out["stream_attention_ms"] / 1e9
    if out["dense_workspace_bytes"] == 0 or out["dense_workspace_bytes"] > DENSE_MAX_WS:
        out["dense_skipped"] = (f"the dense path asks for {out['dense_workspace_bytes']} bytes of workspace, past this script's cap of {DENSE_MAX_WS}: "
                                "not run, not estimated")
    else:
        out["dense_score_ms"], out["dense_score_ms_all"], out["dense_attention_ms"], sd = timed("dense", TAG_DENSE)
        out["dense_attention_tflops"] = flop / out["dense_attention_ms"] / 1e9
        out["dense_over_stream_attention"] = out["dense_attention_ms"] / out["stream_attention_ms"]
        out["dense_over_stream_score"] = out["dense_score_ms"] / out["stream_score_ms"]
        out["stream_attention_not_slower"] = out["stream_attention_ms"] <= out["dense_attention_ms"]
        out["max_abs_stream_minus_dense_scores"] = float((ss - sd).abs().max())
    print("RESULT " + json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "attn_stream_timing.json")
    res = {"box": "1x MI355X", "D": D, "heads": HEADS, "layers": LAYERS, "precision": "fp32",
           "call": "Transformer.score_packed, HIP events around one call; attention launches by the library's profiler", "runs": {}}
    for name, lens in runs():
        spec = {"name": name, "lens": lens, "reps": 5, "warmup": 2}
        if name.endswith("attention_only"):
            spec.update(attention_only=True, D=2048, heads=8)
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
    if "T8192" in res["runs"]:
        res["condition_T8192_stream_attention_not_slower"] = res["runs"]["T8192"].get("stream_attention_not_slower")
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(json.loads(sys.argv[2]))
    else:
        sys.exit(main())
