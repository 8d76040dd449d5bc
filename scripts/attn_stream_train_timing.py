"""Training the Transformer scorer with attention_train="stream" (csrc/attn_stream_bwd.hip: no (T x T) block kept or rebuilt) beside the dense
training step on long videos.

D = 1024, 8 heads of 128 columns, F = D, exact fp32, one video, dropout 0.1 in the layers and 0.5 before the head.  One step is zero_grad +
forward + MSE + backward, without the optimiser:
  * one encoder layer, T = 4096 and 8192: the stream step beside the dense step in the same run (one layer keeps the dense workspace under
    DENSE_MAX_WS: 4.3 GB of alpha blocks at T = 8192);
  * six layers, T = 8192, 16 384, 32 768: the stream step alone with its workspace; the dense query's answer is recorded, the dense step is
    not run and not estimated;
  * in every stream run the launches of the attention one by one through the library's profiler: the training forward, and delta, the dQ
    pass and the dK / dV pass of the backward (means per launch over the steps of a second loop, not part of the timed steps).
Expectation, recorded beside each measurement and measured by nobody: 14 T^2 D FLOP for the two backward passes of one layer at the
122 TFLOP/s the forward launch reached at T = 8192 (profiles/attn_stream_timing.json) -- about 7.9 ms per layer at T = 8192.  That rate was
measured on another kernel with two waves per SIMD, not on these, which run one.
The one condition: at T = 8192 with one layer the stream step takes at most 1.4 times the dense step of the same run (seven products against
five at equal rate); the measured ratio is recorded whatever it is ("stream_over_dense_step", "condition_T8192_L1_ratio_at_most_1.4").
Per run: the median over 5 steps of one step's stream time (HIP events around the step, 2 warm-up steps first).  Every GPU run is a fresh
child of this script under its own time limit; after a run that fails or runs out of time nothing more is started.
    python scripts/attn_stream_train_timing.py [OUT.json]      (writes profiles/attn_stream_train_timing.json by default)"""
import json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HEADS = 1024, 8
STEP_LIMIT_S = 240
DENSE_MAX_WS = 8 * 2 ** 30
FORWARD_TFLOPS = 122.0


def runs():
    return [("L1_T4096", 1, 4096), ("L1_T8192", 1, 8192), ("L6_T8192", 6, 8192), ("L6_T16384", 6, 16384), ("L6_T32768", 6, 32768)]


def worker(spec):
    import ctypes as C
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from summarizer_amd import _lib, kernels
    from summarizer_amd.models.transformer import Transformer
    dev = torch.device("cuda:0")
    T, layers, reps, warm = spec["T"], spec["layers"], spec["reps"], spec["warmup"]
    lib = _lib.load()
    tags = {"train_forward_ms": _lib.PROF_ATTN_STREAM_TRAIN, "backward_delta_ms": _lib.PROF_ATTN_STREAM_BWD_DELTA,
            "backward_dq_ms": _lib.PROF_ATTN_STREAM_BWD_DQ, "backward_dkv_ms": _lib.PROF_ATTN_STREAM_BWD_DKV}      # SUMK_PROF_* of include/sumk.h
    x = (0.5 * torch.randn(T, D, generator=torch.Generator().manual_seed(T))).to(dev)
    target = torch.rand(T, generator=torch.Generator().manual_seed(T + 1)).to(dev)
    sb = kernels.SeqBatch.get([T], dev)
    bwd_flop = 14 * T * T * D
    out = {"T": T, "D": D, "heads": HEADS, "layers": layers, "reps": reps, "warmup": warm, "layer_dropout_p": 0.1, "head_dropout_p": 0.5,
           "backward_passes_flop_per_layer": bwd_flop,
           "expected_backward_passes_ms_per_layer_at_122_tflops": bwd_flop / (FORWARD_TFLOPS * 1e12) * 1e3,
           "expectation_note": "14 T^2 D FLOP at the rate of the forward launch (two waves per SIMD); not measured on these kernels (one wave per SIMD)",
           "stream_workspace_bytes": int(kernels.transformer_workspace_bytes(D, D, HEADS, layers, sb, "stream", training=True)),
           "dense_workspace_bytes": int(lib.sumk_transformer_workspace_bytes(D, D, HEADS, layers, sb.n_seq, sb.off_host_p, 1))}

    def model(att):
        torch.manual_seed(7)
        return Transformer(input_size=D, encoder_layers=layers, attention_heads=HEADS, attention_train=att).to(dev).train()

    def step(m):
        m.zero_grad()
        loss = torch.nn.functional.mse_loss(m.score_packed(x, [T]), target)
        loss.backward()
        return loss

    def timed(m):
        for _ in range(warm):
            loss = step(m)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); loss = step(m); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
        return float(np.median(ts)), [round(t, 3) for t in ts]

    ms_ = model("stream")
    out["stream_step_ms"], out["stream_step_ms_all"] = timed(ms_)
    lib.sumk_prof_enable(sum(1 << t for t in tags.values()))
    for t in tags.values():
        lib.sumk_prof_read(t, None, None, 1)
    for _ in range(reps):
        step(ms_)
    torch.cuda.synchronize()
    for name, t in tags.items():
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        lib.sumk_prof_read(t, C.byref(ms), C.byref(cnt), 1)
        assert cnt.value == reps * layers, (name, cnt.value)
        out["attention_" + name] = ms.value / cnt.value
    lib.sumk_prof_enable(0)
    passes = out["attention_backward_dq_ms"] + out["attention_backward_dkv_ms"]
    out["backward_passes_tflops"] = bwd_flop / passes / 1e9
    out["train_forward_tflops"] = 4 * T * T * D / out["attention_train_forward_ms"] / 1e9
    del ms_
    torch.cuda.empty_cache()
    if layers > 1 or out["dense_workspace_bytes"] > DENSE_MAX_WS:
        out["dense_skipped"] = (f"the dense training step asks for {out['dense_workspace_bytes']} bytes of workspace"
                                + (f", past this script's cap of {DENSE_MAX_WS}" if out["dense_workspace_bytes"] > DENSE_MAX_WS else "")
                                + ": not run, not estimated (the side-by-side runs have one layer)")
    else:
        out["dense_step_ms"], out["dense_step_ms_all"] = timed(model("dense"))
        out["stream_over_dense_step"] = out["stream_step_ms"] / out["dense_step_ms"]
    print("RESULT " + json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "attn_stream_train_timing.json")
    res = {"box": "1x MI355X", "D": D, "heads": HEADS, "precision": "fp32",
           "step": "zero_grad + Transformer.score_packed (training mode) + MSE + backward, HIP events around one step; attention launches by the "
                   "library's profiler", "runs": {}}
    for name, layers, T in runs():
        spec = {"name": name, "layers": layers, "T": T, "reps": 5, "warmup": 2}
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
    ratio = res["runs"].get("L1_T8192", {}).get("stream_over_dense_step")
    if ratio is not None:
        res["T8192_L1_stream_over_dense_step"] = ratio
        res["condition_T8192_L1_ratio_at_most_1.4"] = ratio <= 1.4
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(json.loads(sys.argv[2]))
    else:
        sys.exit(main())
