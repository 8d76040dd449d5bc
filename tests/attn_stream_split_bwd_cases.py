"""The input families of tests/test_gpu_attn_stream_split_bwd.py, built on the host so that tests/test_attn_stream_split_bwd_host.py can
check them without a GPU, and the specifications of a case, computed once and shared.  TEST INFRASTRUCTURE ONLY.

Cases are tests/attn_stream_bwd_cases.py's dicts (imported, not edited) restricted to the head widths the bf16x3 path takes: multiples of
8 up to 128.  The kernels keep the fp32 path's sizes (32-row wave blocks, 64-row tiles, 128-row strips), so the strips walk
attn_stream_cases.STRIP_T unchanged."""
import numpy as np

import attn_stream_bwd_cases as bwd
from attn_stream_split_cases import BF16X3_MULT, STRIP_SHAPES  # noqa: F401  ((32,4), (80,2), (208,2), (128,1), (256,2): dh 8, 40, 104, 128, 128)

fwd = bwd.fwd
SEED, SITE = bwd.SEED, bwd.SITE
STRIP_DROPOUT = ((80, 2), (256, 2))                  # dh = 40 and 128 also run at p = 0.1 and 0.5
TENSORS = ("ctx", "dq", "dk", "dv")
with_grad = bwd.with_grad
_SPEC3 = {}


def strips(D, heads, p):
    return bwd.strips(D, heads, p)


def ragged():
    return bwd.ragged()


def spikes():
    return bwd.spikes()


def families():
    fam = {f"strips_D{D}_h{h}_p0.0": strips(D, h, 0.0) for D, h in STRIP_SHAPES}
    for D, h in STRIP_DROPOUT:
        for p in (0.1, 0.5):
            fam[f"strips_D{D}_h{h}_p{p}"] = strips(D, h, p)
    fam["ragged"] = ragged()
    fam["spike"] = spikes()
    return fam


def spec(c):
    """(float64 reference, fp32 yardstick run, bf16x3 yardstick run) of a case: dicts with ctx, dq, dk, dv; computed once per process."""
    from attn_stream_split_bwd_ref import mha3_train
    if c["name"] not in _SPEC3:
        s64, s32 = bwd.spec(c)
        _SPEC3[c["name"]] = (s64, s32, mha3_train(c["q"], c["k"], c["v"], c["dctx"], c["lens"], c["heads"], fwd.scale_of(c), c["p"], SEED, SITE))
    return _SPEC3[c["name"]]


def yardsticks(fam, which=2):
    """{tensor: the largest |run - float64 reference| over a family's cases (NaN elements apart)}; which: 2 the bf16x3 run, 1 the fp32 run."""
    with np.errstate(invalid="ignore"):
        return {t: max(float(np.nanmax(np.abs(spec(c)[which][t] - spec(c)[0][t]))) for c in fam) for t in TENSORS}
