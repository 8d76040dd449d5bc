"""Probe of the H = 1024 forward recurrence (csrc/lstm.hip: lstm_wide2_kernel vs lstm_wide_kernel): sLSTM scoring on the S-TVSum batch per
precision -- whole call, and the recurrence launches alone (HIP events on the launch stream, sumk_prof_*) -- plus the scores' digest so that
two processes (SUMK_LSTM_WIDE2=1 / 0) can be compared.
usage: python scripts/probes/wide2_probe.py [out.npz]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from summarizer_amd import _lib, kernels
from summarizer_amd.models.sumgan import sLSTM

dev = torch.device("cuda:0")
lib = _lib.load()
rng = np.random.default_rng(0)
lens = [int(v) for v in rng.integers(150, 321, 50)]
lens[0] = 320
frames = sum(lens)
torch.manual_seed(1234)
x = torch.randn(frames, 1024, device=dev) * 0.5
m = sLSTM(input_size=1024).to(dev).eval()
out = {}
for prec in ["fp32", "bf16x6", "bf16x3"]:
    m.precision = prec
    with torch.no_grad():
        for _ in range(3):
            s = m.score_packed(x, lens)
        torch.cuda.synchronize()
        n = 5
        t0 = time.perf_counter()
        for _ in range(n):
            s = m.score_packed(x, lens)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        lib.sumk_prof_enable(1 << 2)
        for _ in range(n):
            s = m.score_packed(x, lens)
        ms, cnt = C.c_double(0), C.c_int64(0)
        lib.sumk_prof_read(2, C.byref(ms), C.byref(cnt), 1)
        lib.sumk_prof_enable(0)
    kernels.health_check()
    out[prec] = s.cpu().numpy()
    print(f"{prec:7s} WIDE2={os.environ.get('SUMK_LSTM_WIDE2', '1')}: whole call {dt * 1e3:7.3f} ms; recurrence {ms.value / max(cnt.value, 1) * 1e3:8.1f} us per layer launch "
          f"= {ms.value / max(cnt.value, 1) * 1e3 / max(lens):6.2f} us per step ({cnt.value} launches)", flush=True)
if out:
    print("max |bf16x6 - fp32| =", float(np.abs(out["bf16x6"] - out["fp32"]).max()), " max |bf16x3 - fp32| =", float(np.abs(out["bf16x3"] - out["fp32"]).max()))
    if len(sys.argv) > 1:
        np.savez(sys.argv[1], **out)
