#!/usr/bin/env python3
"""The VASNet size queries on a grid that sits on both sides of every boundary of the forward's path plan (csrc/vasnet.hip:
plan_forward), recorded from the library of the commit BEFORE the path plan was given one home -- the values a caller allocates by.

Record once, from that library (the queries are pure host arithmetic: no GPU):
    git worktree add <dir> <parent commit> && make -C <dir>/summarizer_amd/csrc
    SUMK_LIB_PATH=<dir>/summarizer_amd/libsumk.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vasnet_workspace.py
tests/test_vasnet_workspace_host.py imports DIMS / LENGTHS / PRECISIONS / PLANES from here: the fixture cannot shrink unnoticed."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (256, 260, 1024)                     # the smallest plane-eligible width, one that is not (D % 256), the model's
PRECISIONS = (0, 1, 2, 3)                   # SUMK_PRECISION_FP32, BF16X3, BF16X6, BF16
PLANES = (0, 1, 2, 3, 4)                    # sumk_vasnet_wplanes_bytes: 2 and 3 are valid plane counts
LENGTHS = {
    "rows_1024": [512, 512], "rows_1025": [512, 513],               # the small-batch limit (SK_MAX_ROWS)
    "rows_255": [100, 155], "rows_256": [100, 156],                 # the plane path's least batch
    "tmax_320": [320, 300, 17], "tmax_321": [321, 300],             # the strip limit of the plane attention
    "tmin_1535": [1535, 1600], "tmin_1536": [1536, 1600],           # PW_LONG_TMIN
    "lone_long": [1600],                                            # rows < Tn: no direct [Q | K] planes
    "ragged": [1, 333, 64, 2000],
}


def offsets(lens):
    off = [0]
    for t in lens:
        off.append(off[-1] + t)
    return (C.c_int32 * len(off))(*off)


def query(lib):
    """Every value of the grid as {key: bytes}; keys are plain strings so the fixture reads as a table."""
    out = {}
    for D in DIMS:
        for n in PLANES:
            out[f"wplanes/D{D}/np{n}"] = int(lib.sumk_vasnet_wplanes_bytes(D, n))
        for tag, lens in LENGTHS.items():
            off = offsets(lens)
            out[f"tables/D{D}/{tag}"] = int(lib.sumk_vasnet_tables_bytes(D, len(lens), off))
            for training in (0, 1):
                out[f"workspace/D{D}/{tag}/train{training}"] = int(lib.sumk_vasnet_workspace_bytes(D, len(lens), off, training))
                for p in PRECISIONS:
                    out[f"workspace_for/D{D}/{tag}/train{training}/prec{p}"] = int(lib.sumk_vasnet_workspace_bytes_for(D, len(lens), off, training, p))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from summarizer_amd import _lib
    values = query(_lib.load())
    path = os.path.join(HERE, "vasnet_workspace.json")
    with open(path, "w") as f:
        json.dump({"library": "parent of the path-plan refactor", "lengths": LENGTHS, "bytes": values}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"vasnet_workspace: {len(values)} values from {_lib.LIB_PATH}, {os.path.getsize(path) / 1024:.1f} KB")
