"""CPU: the size queries of the recurrent layers are pinned, byte for byte, to what the library returned before the LSTM layers were given
one carve for one or two directions and one path plan (csrc/lstm.hip: lstm_carve, which the size queries, the forward and the backward
all read).  A query that promises less than a path then uses is an out-of-bounds write; one that moves at all changes what cached
workspaces of an older call assume.  The grid (tests/golden/make_golden_lstm_workspace.py) sits on both sides of every rule of the plan;
the queries are host arithmetic and need no GPU."""
import json
import os

import pytest

import make_golden_lstm_workspace as mk
from conftest import GOLDEN, ROOT

LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")
MIB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    from summarizer_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "lstm_workspace.json")) as f:
        return json.load(f)


def test_size_queries_equal_the_recorded_bytes(lib, recorded):
    got = mk.query(lib)
    want = recorded["bytes"]
    assert recorded["lengths"] == {str(n): mk.lengths(n) for n in mk.N_SEQ}        # the fixture was recorded on this grid ...
    assert set(got) == set(want) and len(want) == mk.grid_size()                   # ... all of it
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_valid_shapes_have_a_size_and_refused_ones_none(recorded):
    b = recorded["bytes"]
    for k, v in b.items():
        layer = k.split("/")[0]
        if layer == "refused":
            assert v == 0, k
        elif layer == "bigru":
            assert (v > 0) == ("/H260/" not in k), k
        elif layer == "decoder":
            assert (v > 0) == ("/L0/" not in k and "/L9/" not in k), k
        elif layer == "wplanes":
            assert (v > 0) == ("/H256/" in k and "/In128/" in k and k[-3:] in ("np2", "np3")), k
        elif layer == "linear":
            assert (v > 0) == ("N0" not in k and "K0" not in k and "N-4" not in k), k
        else:
            assert v > 0, k


def test_the_grid_sees_every_plan_boundary(recorded):
    """`extra` is what a bidirectional workspace holds beyond two one-direction ones: the blocks of the persistent kernels (state words,
    forward hand-off or wide exchange; in training also the BPTT's state words and exchange), less one GEMM descriptor block and, in
    training past 8 videos, less the two mat-vec blocks that only the one-direction layer carries at every batch size.  Each assertion
    straddles one rule of the plan with a margin far above the 256-byte alignment of the blocks, so a rule that drifts moves a pinned
    value."""
    b = recorded["bytes"]
    In = mk.INPUTS[0]
    extra = lambda H, n, t: b[f"bilstm/H{H}/n{n}/In{In}/train{t}"] - 2 * b[f"lstm/H{H}/n{n}/In{In}/train{t}"]
    train = lambda H, n: extra(H, n, 1) - extra(H, n, 0)                # the BPTT's blocks alone
    # H <= 256: the hand-off buffer (32 n H bytes); 256 < H <= 1024: the wide exchange, 1 MiB per group of 64 videos; above: neither
    assert extra(256, 1, 0) < MIB <= extra(260, 1, 0)
    assert extra(1028, 1, 0) < MIB <= extra(1024, 1, 0)
    for H in (320, 384, 1024):
        assert extra(H, 65, 0) - extra(H, 64, 0) >= MIB, H               # 64 vs 65 videos: a second wide group
    assert extra(256, 65, 0) - extra(256, 64, 0) < MIB
    # wide BPTT exchange (H % 128 == 0): 8 (H / 32) 64 H floats = 9 MiB at 384, nothing at 320
    assert train(384, 64) > 4 * MIB > train(320, 64)
    # the small-batch mat-vec block of the bidirectional layer: there at 8 videos (and twice the one-direction one), gone at 9
    assert train(320, 8) > 0 > train(320, 9)
    # H <= 256 BPTT exchange, 2 x items x 32 x 32 x H floats: 128 videos are 4 groups of 32, 129 are 5 -- two more items
    for H in (252, 256):
        assert abs(train(H, 129) - train(H, 128) - 2 * 2 * 32 * 32 * H * 4) <= 1024, H
    # the slab of the weight gradients takes the larger of In and H
    for H in mk.HIDDEN:
        for layer in ("bilstm", "lstm"):
            lo, hi = (b[f"{layer}/H{H}/n9/In{i}/train1"] - b[f"{layer}/H{H}/n9/In{i}/train0"] for i in mk.INPUTS)
            assert hi > lo, (layer, H)
