"""One VASNet TRAINING step with the attention on the band (VASNet(local_attention_train="band"), csrc/attn_band_bwd.hip) beside the dense
masked path on one long video.

One video at D = 1024, exact fp32, dropout 0.5.  A step is zero_grad + forward (score_packed) + per-video MSE + backward, no optimiser:
  * T = 4096 and 16384 at w = 64 and 256: both paths and their ratio;
  * T = 65536 at w = 64 and 256: the band alone.  The dense run is skipped there -- its training workspace query answers more than
    DENSE_MAX_WS (two (T x T) blocks alone are 32 GiB) -- and the record says so with the bytes it asked for;
  * at T = 65536, w = 256 the seven launches of the attention backward separately (event pairs of the library's profiler around each).
Expectation, recorded beside each measured ratio: the per-video products shrink by T / (2 w + 64), while the row-wise GEMMs (18 T D^2 FLOP,
forward + backward) do not.  The one condition: at T = 16384, w = 256 the band step is not slower than the dense step ("band_not_slower").
Per run: the median over 5 steps of one step's stream time (HIP events around the step, 2 warm-up steps first).  Every GPU step is a fresh
child of this script under its own time limit; after a step that fails or runs out of time nothing more is started.
    python scripts/attn_band_train_timing.py [OUT.json]      (writes profiles/attn_band_train_timing.json by default)"""
import json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 1024
STEP_LIMIT_S = 240
DENSE_MAX_WS = 8 * 2 ** 30
RUNS = [(4096, 64), (4096, 256), (16384, 64), (16384, 256), (65536, 64), (65536, 256)]
BREAKDOWN = (65536, 256)
TAGS = {"transpose_alphaD_ms": 8, "dV_ms": 9, "dAlphaD_ms": 10, "softmax_backward_ms": 11, "dQ_ms": 12, "transpose_dLogits_ms": 13,
        "dK_ms": 14}      # SUMK_PROF_BAND_BWD_* (include/sumk.h), in launch order


def worker(spec):
    import ctypes as C
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from summarizer_amd import _lib, kernels
    from summarizer_amd.autograd import SegmentMseMeanFunction
    from summarizer_amd.models.vasnet import VASNet
    dev = torch.device("cuda:0")
    T, w, reps, warm = spec["T"], spec["w"], spec["reps"], spec["warmup"]
    lib = _lib.load()
    torch.manual_seed(1)
    band = VASNet(input_size=D, attention_aperture=w, local_attention="band", local_attention_train="band").train()
    dense = VASNet(input_size=D, attention_aperture=w).train()
    dense.load_state_dict(band.state_dict())
    band, dense = band.to(dev), dense.to(dev)
    x = (0.5 * torch.randn(T, D, generator=torch.Generator().manual_seed(T + w)).abs()).to(dev)      # pool5-like non-negative features
    target = torch.rand(T, generator=torch.Generator().manual_seed(7)).to(dev)
    sb = kernels.SeqBatch.get([T], dev)
    out = {"T": T, "w": w, "reps": reps, "warmup": warm, "dropout_p": 0.5, "flop_ratio_T_over_2w_plus_64": T / (2 * w + 64),
           "rowwise_gemm_flop": 18 * T * D * D,
           "band_workspace_bytes": int(kernels.vasnet_band_train_workspace_bytes(D, sb, w)),
           "dense_workspace_bytes": int(lib.sumk_vasnet_workspace_bytes(D, 1, sb.off_host_p, 1))}

    def step(model):
        for p in model.parameters():
            if p.grad is not None:
                p.grad.zero_()
        loss = SegmentMseMeanFunction.apply(model.score_packed(x, [T]), target, sb, 1.0)
        loss.backward(gradient=kernels.one_for(loss))
        return loss.detach()

    def timed(model):
        for _ in range(warm):
            step(model)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); loss = step(model); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        return float(np.median(ts)), [round(t, 3) for t in ts]

    out["band_ms"], out["band_ms_all"] = timed(band)
    if (T, w) == BREAKDOWN:      # the seven launches, on steps of their own (not part of the timed steps above)
        lib.sumk_prof_enable(sum(1 << t for t in TAGS.values()))
        for t in TAGS.values():
            lib.sumk_prof_read(t, None, None, 1)
        for _ in range(reps):
            step(band)
        torch.cuda.synchronize()
        for name, t in TAGS.items():
            ms, n = C.c_double(0.0), C.c_int64(0)
            lib.sumk_prof_read(t, C.byref(ms), C.byref(n), 1)
            out[name] = ms.value / max(n.value, 1)
        lib.sumk_prof_enable(0)
    if out["dense_workspace_bytes"] == 0 or out["dense_workspace_bytes"] > DENSE_MAX_WS:
        out["dense_skipped"] = (f"the dense path asks for {out['dense_workspace_bytes']} bytes of workspace (two (T x T) blocks alone are {8 * T * T}), "
                                f"past this script's cap of {DENSE_MAX_WS}: not run, not estimated")
    else:
        out["dense_ms"], out["dense_ms_all"] = timed(dense)
        out["dense_over_band"] = out["dense_ms"] / out["band_ms"]
        out["band_not_slower"] = out["band_ms"] <= out["dense_ms"]
    print("RESULT " + json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "attn_band_train_timing.json")
    res = {"box": "1x MI355X", "D": D, "precision": "fp32", "step": "zero_grad + forward + MSE + backward, no optimiser", "runs": {}}
    for T, w in RUNS:
        spec = {"T": T, "w": w, "reps": 5, "warmup": 2}
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(spec)], capture_output=True, text=True,
                               timeout=STEP_LIMIT_S, cwd=ROOT)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"T={T} w={w}: no result within {STEP_LIMIT_S} s; nothing more was started"
            break
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res["stopped"] = f"T={T} w={w}: exit code {r.returncode}; nothing more was started: {r.stderr[-600:]}"
            break
        res["runs"][f"T{T}_w{w}"] = json.loads(line[-1][7:])
        print(f"T={T} w={w}: " + line[-1][7:], flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(json.loads(sys.argv[2]))
    else:
        sys.exit(main())
