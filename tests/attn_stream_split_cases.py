"""The input families of tests/test_gpu_attn_stream_split.py, built on the host so that tests/test_attn_stream_split_host.py can check them
without a GPU, and the specifications of a case, computed once and shared.  TEST INFRASTRUCTURE ONLY.

Cases are tests/attn_stream_cases.py's dicts.  The bf16x3 kernel keeps the fp32 kernel's sizes (32-row wave blocks, 64-key tiles, 128-row
strips), so the strips walk attn_stream_cases.STRIP_T unchanged; its head widths are multiples of 8 up to 128."""
import numpy as np

import attn_stream_cases as base
from attn_stream_ref import mha
from attn_stream_split_ref import mha3

STRIP_SHAPES = ((32, 4), (80, 2), (208, 2), (128, 1), (256, 2))      # (D, heads): dh = 8, 40, 104, 128, 128
BF16X3_MULT = 4.0 * 2.0 ** 8        # tests/test_gpu_vasnet_lengths.py: an x3 yardstick may be this many fp32 yardsticks at most
_SPEC = {}


def strips(D, heads):
    return base.strips(D, heads)


def families():
    fam = {f"strips_D{D}_h{h}": strips(D, h) for D, h in STRIP_SHAPES}
    fam["ragged"] = base.ragged()
    fam["spike"] = base.spikes()
    return fam


def spec(c):
    """(ctx64, lse64, ctx32, lse32, ctx3, lse3) of a case: the float64 reference, the fp32 yardstick run, the bf16x3 yardstick run."""
    if c["name"] not in _SPEC:
        sc = base.scale_of(c)
        a = (c["q"], c["k"], c["v"], c["lens"], c["heads"], sc)
        _SPEC[c["name"]] = mha(*a) + mha(*a, np.float32) + mha3(*a)
    return _SPEC[c["name"]]


def yardsticks(fam):
    """(x3 ctx, x3 lse, fp32 ctx, fp32 lse): the largest |run - float64 reference| over a family's cases (NaN elements apart)."""
    with np.errstate(invalid="ignore"):
        d = lambda i, j: max(float(np.nanmax(np.abs(spec(c)[i] - spec(c)[j]))) for c in fam)
        return d(4, 0), d(5, 1), d(2, 0), d(3, 1)
