"""Probe of `DSN(cell="gru")` next to the LSTM cell of the same model: scoring and one MSE training step (zero_grad + forward +
backward + Adam) on the 50-video batch of tests/test_gpu_gru_persist.py and on one 300-frame video per call.  HIP events, 5 warm-up
and 20 timed iterations, median and p10 / p90 in ms; prints ONE JSON line.  Uses only the models' public interface, so it also runs on
a tree that predates the persistent GRU kernels:  python scripts/probes/gru_probe.py [--tree OTHER_CHECKOUT] [--label NAME]."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--label", default="this tree")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import ctypes as C
import numpy as np
import torch
from summarizer_amd import _lib, kernels
from summarizer_amd.models.dsn import DSN

dev = torch.device("cuda:0")
D, H = 1024, 256


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    q = np.percentile(ms, [50, 10, 90])
    return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}


def recurrence_us(fn):
    """Mean time of the forward recurrence launch alone (the library's event pairs), or None where the path has no such launch."""
    lib = _lib.load()
    lib.sumk_prof_enable(1 << 2)
    for _ in range(args.iters):
        fn()
    ms, cnt = C.c_double(0), C.c_int64(0)
    lib.sumk_prof_read(2, C.byref(ms), C.byref(cnt), 1)
    lib.sumk_prof_enable(0)
    return round(ms.value / cnt.value * 1e3, 2) if cnt.value else None


batches = {"50_videos": [int(v) for v in np.ceil(np.random.default_rng(0).uniform(150, 320, 50))], "1_video_300": [300]}
out = {"label": args.label, "D": D, "H": H, "warmup": args.warmup, "iters": args.iters}
for cell in ("gru", "lstm"):
    torch.manual_seed(7)
    m = DSN(D, H, 1, cell=cell).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-5)
    for name, lens in batches.items():
        g = torch.Generator().manual_seed(11)
        x = (torch.randn(sum(lens), D, generator=g) * 0.5).to(dev)
        target = torch.rand(sum(lens), generator=g).to(dev)

        def score():
            with torch.no_grad():
                return m.score_packed(x, lens)

        def train():
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(m.score_packed(x, lens), target)
            loss.backward()
            opt.step()

        r = {"score": timed(score), "train": timed(train)}
        us = recurrence_us(score)
        if us is not None:
            r["score_recurrence_us"] = us
            r["score_recurrence_us_per_step"] = round(us / max(lens), 3)
        out[f"{cell}/{name}"] = r
        kernels.health_check()
print(json.dumps(out), flush=True)
