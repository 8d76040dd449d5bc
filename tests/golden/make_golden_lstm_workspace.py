#!/usr/bin/env python3
"""The size queries of the recurrent layers (csrc/lstm.hip, csrc/gru_persist.hip) on a grid that sits on both sides of every rule of
the LSTM path plan (lstm.hip: lstm_carve), recorded from the library of the commit BEFORE the carves and the plan were given one home
-- the values a caller allocates by.

Record once, from that library (the queries are pure host arithmetic: no GPU):
    git worktree add <dir> <parent commit> && make -C <dir>/summarizer_amd/csrc
    SUMK_LIB_PATH=<dir>/summarizer_amd/libsumk.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lstm_workspace.py
tests/test_lstm_workspace_host.py imports the grid from here: the fixture cannot shrink unnoticed."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HIDDEN = (252, 256, 260, 320, 384, 1024, 1028)   # persistent (H <= 256) | wide (<= 1024; BPTT: H % 128 == 0) | launch chain
N_SEQ = (1, 8, 9, 64, 65, 128, 129)              # mat-vec limit 8 | wide groups of 64 | persistent groups of 32 at 16 per item
INPUTS = (64, 1040)                              # below and above every H: the split-K slab takes the larger of In and H
TRAINING = (0, 1)
GRU_HIDDEN = (252, 256, 260)                     # 260: refused (the persistent GRU serves H <= 256)
DEC_HIDDEN = (256, 260, 1028)
DEC_LAYERS = (0, 1, 2, 8, 9)                     # 0 and 9: refused
DEC_N_SEQ = (1, 8, 9, 129)
PLANES = (1, 2, 3, 4)                            # sumk_bilstm_wplanes_bytes: 2 and 3 are valid plane counts
PLANE_INPUTS = (96, 128, 144)                    # below the least width | eligible | not a multiple of 32
PLANE_HIDDEN = (256, 260)                        # 8 x 260 is no multiple of 256
LINEAR = ((4, 4), (1024, 500), (500, 1024), (0, 4), (4, 0), (-4, 4))   # (N, K); the last three: refused
FRAME_HEAD = (4, 512)
# (In, H, seq_off) that every layer's query refuses with 0 (the decoder takes H and seq_off at two layers)
REFUSED = {
    "in_not_4": (66, 256, [0, 3, 5]), "h_not_4": (64, 254, [0, 3, 5]), "off0_not_0": (64, 256, [1, 3, 5]),
    "empty_video": (64, 256, [0, 3, 3, 5]),
}


def lengths(n):
    """n short ragged videos, the first of one frame."""
    return [1 + (3 * i) % 7 for i in range(n)]


def offsets(lens):
    off = [0]
    for t in lens:
        off.append(off[-1] + t)
    return (C.c_int32 * len(off))(*off)


def query(lib):
    """Every value of the grid as {key: bytes}; keys are plain strings so the fixture reads as a table."""
    out = {}
    for n in N_SEQ:
        off = offsets(lengths(n))
        for In in INPUTS:
            for t in TRAINING:
                for H in HIDDEN:
                    out[f"bilstm/H{H}/n{n}/In{In}/train{t}"] = int(lib.sumk_bilstm_workspace_bytes(In, H, n, off, t))
                    out[f"lstm/H{H}/n{n}/In{In}/train{t}"] = int(lib.sumk_lstm_workspace_bytes(In, H, n, off, t))
                for H in GRU_HIDDEN:
                    out[f"bigru/H{H}/n{n}/In{In}/train{t}"] = int(lib.sumk_bigru_workspace_bytes(In, H, n, off, t))
    for n in DEC_N_SEQ:
        off = offsets(lengths(n))
        for H in DEC_HIDDEN:
            for layers in DEC_LAYERS:
                out[f"decoder/H{H}/L{layers}/n{n}"] = int(lib.sumk_lstm_decoder_workspace_bytes(H, layers, n, off))
    for H in PLANE_HIDDEN:
        for In in PLANE_INPUTS:
            for p in PLANES:
                out[f"wplanes/H{H}/In{In}/np{p}"] = int(lib.sumk_bilstm_wplanes_bytes(In, H, p))
    for N, K in LINEAR:
        out[f"linear/N{N}/K{K}"] = int(lib.sumk_linear_workspace_bytes(N, K))
    for F in FRAME_HEAD:
        out[f"frame_head/F{F}"] = int(lib.sumk_frame_head_workspace_bytes(F))
    for tag, (In, H, off) in REFUSED.items():
        n, off = len(off) - 1, (C.c_int32 * len(off))(*off)
        for t in TRAINING:
            out[f"refused/{tag}/bilstm/train{t}"] = int(lib.sumk_bilstm_workspace_bytes(In, H, n, off, t))
            out[f"refused/{tag}/lstm/train{t}"] = int(lib.sumk_lstm_workspace_bytes(In, H, n, off, t))
            out[f"refused/{tag}/bigru/train{t}"] = int(lib.sumk_bigru_workspace_bytes(In, H, n, off, t))
        if tag != "in_not_4":                              # the decoder has no input size
            out[f"refused/{tag}/decoder"] = int(lib.sumk_lstm_decoder_workspace_bytes(H, 2, n, off))
    return out


def grid_size():
    per_batch = len(INPUTS) * len(TRAINING) * (2 * len(HIDDEN) + len(GRU_HIDDEN))
    return (len(N_SEQ) * per_batch + len(DEC_N_SEQ) * len(DEC_HIDDEN) * len(DEC_LAYERS) + len(PLANE_HIDDEN) * len(PLANE_INPUTS) * len(PLANES)
            + len(LINEAR) + len(FRAME_HEAD) + len(REFUSED) * 3 * len(TRAINING) + len(REFUSED) - 1)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from summarizer_amd import _lib
    values = query(_lib.load())
    assert len(values) == grid_size(), (len(values), grid_size())
    path = os.path.join(HERE, "lstm_workspace.json")
    with open(path, "w") as f:
        json.dump({"library": "parent of the LSTM path-plan refactor", "lengths": {str(n): lengths(n) for n in N_SEQ}, "bytes": values}, f,
                  indent=0, sort_keys=True)
        f.write("\n")
    print(f"lstm_workspace: {len(values)} values from {_lib.LIB_PATH}, {os.path.getsize(path) / 1024:.1f} KB")
