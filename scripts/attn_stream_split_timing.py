"""The Transformer scorer on the stream path with its attention in bf16x3 (csrc/attn_stream_split.hip) beside the exact fp32 stream launch
(csrc/attn_stream.hip) on long videos.

D = 1024, 8 heads of 128 columns, F = D, 6 layers, projections exact fp32 both ways, one video at T = 4096 / 8192 / 16384 / 65536 and the
50-video S-TVSum shape (T ~ U(150, 320)).  Per run, both paths in the same process:
  * the attention of one layer: the fp32 stream launch against the split call = the pass that splits Q, K, V into bf16 planes + the bf16x3
    attention launch, each by the library's profiler tags inside the same 6-layer scoring calls;
  * the whole score_packed both ways, and the workspace both ways.
Expectation, recorded beside each measurement: the split call does 4 T^2 D FLOP three times over; at the 1.6 to 1.8 PFLOP/s the box sustains
on random bf16 operands that is about 31 ms per layer at T = 65536 -- but the softmax's vector work does not shrink and the P split adds to
it, so the guess was 2x to 3.5x on the attention launch at long T, less at T = 4096.  Nobody had measured it.  The one condition: at
T = 8192 the split call (split pass + attention) takes no longer per layer than the fp32 stream launch in the same run
("split_attention_not_slower").
Per run: the median over 5 calls of one call's stream time (HIP events around the call, 2 warm-up calls first); per-launch figures are the
profiler's mean over those calls' launches.  Every GPU step is a fresh child of this script under its own time limit; after a step that
fails or runs out of time nothing more is started.
    python scripts/attn_stream_split_timing.py [OUT.json]      (writes profiles/attn_stream_split_timing.json by default)"""
import json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HEADS, LAYERS = 1024, 8, 6
STEP_LIMIT_S = 240
BF16_RANDOM_PFLOPS = 1.7


def runs():
    import numpy as np
    tvsum = [int(t) for t in np.random.default_rng(11).integers(150, 321, size=50)]
    return [("T4096", [4096]), ("T8192", [8192]), ("T16384", [16384]), ("T65536", [65536]), ("s_tvsum_50", tvsum)]


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
    n = sum(lens)
    models = {}
    for prec in ("fp32", "bf16x3"):
        torch.manual_seed(7)
        models[prec] = Transformer(input_size=D, encoder_layers=LAYERS, attention_heads=HEADS, attention="stream",
                                   attention_precision=prec).to(dev).eval()
    models["bf16x3"].load_state_dict(models["fp32"].state_dict())
    x = (0.5 * torch.randn(n, D, generator=torch.Generator().manual_seed(n))).to(dev)
    sb = kernels.SeqBatch.get(lens, dev)
    flop = sum(4 * T * T * D for T in lens)
    out = {"lens": lens if len(lens) < 8 else f"{len(lens)} videos, {n} steps", "D": D, "heads": HEADS, "layers": LAYERS, "reps": reps, "warmup": warm,
           "attention_flop_per_layer": flop, "split_mfma_flop_per_layer": 3 * flop,
           "expected_split_attention_ms_at_1p7_pflops": 3 * flop / (BF16_RANDOM_PFLOPS * 1e15) * 1e3,
           "expectation_note": "3 x 4 T^2 D FLOP at the sustained random-operand bf16 MFMA rate; MFMA time alone, not measured on this kernel",
           "fp32_workspace_bytes": int(kernels.transformer_workspace_bytes(D, D, HEADS, LAYERS, sb, "stream")),
           "split_workspace_bytes": int(kernels.transformer_workspace_bytes(D, D, HEADS, LAYERS, sb, "stream", attention_precision="bf16x3"))}

    def timed(prec, tags):
        m = models[prec]
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
            mask = 0
            for t in tags:
                mask |= 1 << t
            lib.sumk_prof_enable(mask)
            for t in tags:
                lib.sumk_prof_read(t, None, None, 1)
            for _ in range(reps):
                m.score_packed(x, lens)
            torch.cuda.synchronize()
            per = []
            for t in tags:
                ms, cnt = C.c_double(0.0), C.c_int64(0)
                lib.sumk_prof_read(t, C.byref(ms), C.byref(cnt), 1)
                assert cnt.value == reps * LAYERS, (t, cnt.value, reps, LAYERS)
                per.append(ms.value / cnt.value)
            lib.sumk_prof_enable(0)
        return float(np.median(ts)), [round(t, 3) for t in ts], per, s

    out["fp32_score_ms"], out["fp32_score_ms_all"], (out["fp32_attention_ms"],), sf = timed("fp32", (_lib.PROF_ATTN_STREAM,))
    out["split_score_ms"], out["split_score_ms_all"], (out["split_planes_ms"], out["split_attention_launch_ms"]), ss = \
        timed("bf16x3", (_lib.PROF_ATTN_STREAM_SPLIT_PLANES, _lib.PROF_ATTN_STREAM_SPLIT))
    out["split_call_ms"] = out["split_planes_ms"] + out["split_attention_launch_ms"]
    out["fp32_attention_tflops"] = flop / out["fp32_attention_ms"] / 1e9
    out["split_call_effective_tflops"] = flop / out["split_call_ms"] / 1e9
    out["split_launch_mfma_tflops"] = 3 * flop / out["split_attention_launch_ms"] / 1e9
    out["fp32_over_split_attention"] = out["fp32_attention_ms"] / out["split_call_ms"]
    out["fp32_over_split_score"] = out["fp32_score_ms"] / out["split_score_ms"]
    out["split_attention_not_slower"] = out["split_call_ms"] <= out["fp32_attention_ms"]
    out["max_abs_split_minus_fp32_scores"] = float((ss - sf).abs().max())
    print("RESULT " + json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "attn_stream_split_timing.json")
    res = {"box": "1x MI355X", "D": D, "heads": HEADS, "layers": LAYERS, "projections": "fp32", "attention": "fp32 stream | bf16x3 stream",
           "call": "Transformer.score_packed, HIP events around one call; attention launches by the library's profiler", "runs": {}}
    for name, lens in runs():
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
    if "T8192" in res["runs"]:
        res["condition_T8192_split_attention_not_slower"] = res["runs"]["T8192"].get("split_attention_not_slower")
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(json.loads(sys.argv[2]))
    else:
        sys.exit(main())
