"""The input families of tests/test_gpu_attn_stream_bwd.py, built on the host so that tests/test_attn_stream_bwd_host.py can check them without
a GPU.  TEST INFRASTRUCTURE ONLY.

A case is one of tests/attn_stream_cases.py (imported, not edited) with three more keys: dctx (float32 (sum(lens), D), standard normal),
p (the dropout probability of the weights) and name (the forward case's name + "_p<p>").  SEED and SITE are the dropout seed and site of
every case.  A family is a list of cases that share one yardstick."""
import zlib

import numpy as np

import attn_stream_cases as fwd

SEED, SITE = 0x5EED1234, 7
STRIP_SHAPES = ((16, 4), (32, 4), (72, 2), (200, 2), (128, 1), (256, 2))      # (D, heads): dh = 4, 8, 36, 100, 128, 128
STRIP_DROPOUT = ((72, 2), (256, 2))                                           # dh = 36 and 128 also run at p = 0.1 and 0.5


def with_grad(c, p):
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    d = dict(c, name=f"{c['name']}_p{p}", p=float(p))
    d["dctx"] = rng.standard_normal(c["q"].shape).astype(np.float32)
    return d


def strips(D, heads, p):
    return [with_grad(c, p) for c in fwd.strips(D, heads)]


def ragged():
    return [with_grad(c, 0.1) for c in fwd.ragged()]


def spikes():
    return [with_grad(c, 0.0) for c in fwd.spikes()]


def families():
    fam = {f"strips_D{D}_h{h}_p0.0": strips(D, h, 0.0) for D, h in STRIP_SHAPES}
    for D, h in STRIP_DROPOUT:
        for p in (0.1, 0.5):
            fam[f"strips_D{D}_h{h}_p{p}"] = strips(D, h, p)
    fam["ragged"] = ragged()
    fam["spike"] = spikes()
    return fam


_SPEC = {}


def spec(c):
    """(float64 run, float32 run) of tests/attn_stream_bwd_ref.mha_train on a case, computed once per process."""
    from attn_stream_bwd_ref import mha_train
    if c["name"] not in _SPEC:
        a = (c["q"], c["k"], c["v"], c["dctx"], c["lens"], c["heads"], fwd.scale_of(c), c["p"], SEED, SITE)
        _SPEC[c["name"]] = (mha_train(*a), mha_train(*a, dtype=np.float32))
    return _SPEC[c["name"]]
