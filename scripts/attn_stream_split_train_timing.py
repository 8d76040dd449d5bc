"""Training the Transformer scorer with attention_train="stream", attention_train_precision="bf16x3" (csrc/attn_stream_split.hip's training
form, csrc/attn_stream_split_bwd.hip) beside the exact-fp32 stream training step (csrc/attn_stream.hip, csrc/attn_stream_bwd.hip) on long
videos.

D = 1024, 8 heads of 128 columns, F = D, one video, dropout 0.1 in the layers and 0.5 before the head; projections and everything but the
attention products exact fp32 in both.  One step is zero_grad + forward + MSE + backward, without the optimiser:
  * one encoder layer, T = 4096 and 8192: the bf16x3 step beside the fp32 stream step in the same run;
  * six layers, T = 8192, 16 384, 32 768: the bf16x3 step alone;
  * in every run the new launches one by one through the library's profiler: the forward's split pass and the training forward, and the
    backward's split pass, delta (the fp32 launch), the dQ pass and the dK / dV pass (means per launch over the steps of a second loop,
    not part of the timed steps); in the side-by-side runs the four fp32 launches too;
  * the workspace both ways.
Expectation, recorded beside each measurement and measured by nobody: seven products of 2 T^2 D on three bf16 MFMAs each = 42 T^2 D FLOP per
layer, about 2.4 ms at T = 8192 at the 1.2 PFLOP/s the bf16x3 scoring launch reaches (profiles/attn_stream_split_timing.json).  That rate is
of another kernel at two waves per SIMD; the backward passes run one wave per SIMD and carry the hash and two register splits, so expect
them below it.
The one condition: at T = 8192 with one layer the bf16x3 step is no slower than the fp32 stream step of the same run; the measured ratio is
recorded whatever it is ("bf16x3_over_fp32_step", "condition_T8192_L1_bf16x3_no_slower").
Per run: the median over 5 steps of one step's time (HIP events around the step, 2 warm-up steps first).  Every GPU run is a fresh child of
this script under its own time limit; after a run that fails or runs out of time nothing more is started.
    python scripts/attn_stream_split_train_timing.py [OUT.json]      (writes profiles/attn_stream_split_train_timing.json by default)"""
import json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HEADS = 1024, 8
STEP_LIMIT_S = 240
SCORING_PFLOPS = 1.2


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
    tags3 = {"forward_planes_ms": _lib.PROF_ATTN_STREAM_SPLIT_PLANES, "train_forward_ms": _lib.PROF_ATTN_STREAM_SPLIT_TRAIN,
             "backward_planes_ms": _lib.PROF_ATTN_STREAM_SPLIT_BWD_PLANES, "backward_delta_ms": _lib.PROF_ATTN_STREAM_BWD_DELTA,
             "backward_dq_ms": _lib.PROF_ATTN_STREAM_SPLIT_BWD_DQ, "backward_dkv_ms": _lib.PROF_ATTN_STREAM_SPLIT_BWD_DKV}
    tags32 = {"train_forward_ms": _lib.PROF_ATTN_STREAM_TRAIN, "backward_delta_ms": _lib.PROF_ATTN_STREAM_BWD_DELTA,
              "backward_dq_ms": _lib.PROF_ATTN_STREAM_BWD_DQ, "backward_dkv_ms": _lib.PROF_ATTN_STREAM_BWD_DKV}
    x = (0.5 * torch.randn(T, D, generator=torch.Generator().manual_seed(T))).to(dev)
    target = torch.rand(T, generator=torch.Generator().manual_seed(T + 1)).to(dev)
    sb = kernels.SeqBatch.get([T], dev)
    flop = 42 * T * T * D
    out = {"T": T, "D": D, "heads": HEADS, "layers": layers, "reps": reps, "warmup": warm, "layer_dropout_p": 0.1, "head_dropout_p": 0.5,
           "attention_mfma_flop_per_layer": flop,
           "expected_attention_ms_per_layer_at_1.2_pflops": flop / (SCORING_PFLOPS * 1e15) * 1e3,
           "expectation_note": "42 T^2 D FLOP at the rate of the bf16x3 scoring launch (two waves per SIMD); not measured on these kernels",
           "bf16x3_workspace_bytes": int(kernels.transformer_workspace_bytes(D, D, HEADS, layers, sb, "stream", training=True,
                                                                             attention_train_precision="bf16x3")),
           "fp32_stream_workspace_bytes": int(kernels.transformer_workspace_bytes(D, D, HEADS, layers, sb, "stream", training=True))}

    def model(prec):
        torch.manual_seed(7)
        return Transformer(input_size=D, encoder_layers=layers, attention_heads=HEADS, attention_train="stream",
                           attention_train_precision=prec).to(dev).train()

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

    def launches(m, tags, prefix):
        lib.sumk_prof_enable(sum(1 << t for t in tags.values()))
        for t in tags.values():
            lib.sumk_prof_read(t, None, None, 1)
        for _ in range(reps):
            step(m)
        torch.cuda.synchronize()
        total = 0.0
        for name, t in tags.items():
            ms, cnt = C.c_double(0.0), C.c_int64(0)
            lib.sumk_prof_read(t, C.byref(ms), C.byref(cnt), 1)
            assert cnt.value == reps * layers, (name, cnt.value)
            out[prefix + name] = ms.value / cnt.value
            total += ms.value / cnt.value
        lib.sumk_prof_enable(0)
        out[prefix + "launches_ms_per_layer"] = total

    m3 = model("bf16x3")
    out["bf16x3_step_ms"], out["bf16x3_step_ms_all"] = timed(m3)
    launches(m3, tags3, "bf16x3_attention_")
    out["bf16x3_attention_pflops"] = flop / out["bf16x3_attention_launches_ms_per_layer"] / 1e12
    del m3
    torch.cuda.empty_cache()
    if layers == 1:
        m32 = model("fp32")
        out["fp32_stream_step_ms"], out["fp32_stream_step_ms_all"] = timed(m32)
        launches(m32, tags32, "fp32_attention_")
        out["bf16x3_over_fp32_step"] = out["bf16x3_step_ms"] / out["fp32_stream_step_ms"]
    print("RESULT " + json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "attn_stream_split_train_timing.json")
    res = {"box": "1x MI355X", "D": D, "heads": HEADS, "attention_train_precision": "bf16x3",
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
    ratio = res["runs"].get("L1_T8192", {}).get("bf16x3_over_fp32_step")
    if ratio is not None:
        res["T8192_L1_bf16x3_over_fp32_step"] = ratio
        res["condition_T8192_L1_bf16x3_no_slower"] = ratio <= 1.0
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(json.loads(sys.argv[2]))
    else:
        sys.exit(main())
