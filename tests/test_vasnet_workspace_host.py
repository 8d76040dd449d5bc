"""CPU: the VASNet size queries are pinned, byte for byte, to what the library returned before the forward's path choice, its workspace
need and the size query were given one plan (csrc/vasnet.hip: plan_forward and the predicates it shares with
sumk_vasnet_workspace_bytes_for).  A query that promises less than the forward then uses is an out-of-bounds write; one that moves at
all changes what `opts->tables` blocks and cached workspaces of an older call assume.  The grid (tests/golden/
make_golden_vasnet_workspace.py) sits on both sides of every boundary of the plan; the queries are host arithmetic and need no GPU."""
import json
import os

import pytest

import make_golden_vasnet_workspace as mk
from conftest import GOLDEN, ROOT

LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    from summarizer_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "vasnet_workspace.json")) as f:
        return json.load(f)


def test_size_queries_equal_the_recorded_bytes(lib, recorded):
    got = mk.query(lib)
    want = recorded["bytes"]
    assert recorded["lengths"] == mk.LENGTHS                       # the fixture was recorded on this grid ...
    assert set(got) == set(want) and len(want) == len(mk.DIMS) * (len(mk.PLANES) + len(mk.LENGTHS) * (1 + 2 + 2 * len(mk.PRECISIONS)))   # ... all of it
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert all(v > 0 for k, v in want.items() if not k.startswith("wplanes/"))       # every batch of the grid is a valid one


def test_the_grid_sees_every_plan_boundary(recorded):
    """Each pair of length lists straddles one predicate: at the plane-eligible widths the recorded size of the plane precisions (inference)
    is NOT what the plain carve-up gives on one side at least, so a predicate that drifts moves a pinned value; at D = 260 (no planes) the
    precision never matters."""
    b = recorded["bytes"]
    for D in (256, 1024):
        for p in (1, 2):
            extra = lambda tag: b[f"workspace_for/D{D}/{tag}/train0/prec{p}"] - b[f"workspace_for/D{D}/{tag}/train0/prec0"]
            assert extra("rows_255") == 0 < extra("rows_256"), (D, p)                       # R >= 256
            assert extra("tmax_320") != extra("tmax_321") and extra("tmax_320") > 0, (D, p)  # strips, then not
            assert extra("tmin_1535") == 0 < extra("tmin_1536"), (D, p)                     # PW_LONG_TMIN
            assert extra("lone_long") > 0 and extra("ragged") == 0, (D, p)
        for tag in mk.LENGTHS:
            assert b[f"workspace_for/D{D}/{tag}/train1/prec1"] == b[f"workspace_for/D{D}/{tag}/train1/prec0"]      # training: never on planes
    assert b["tables/D1024/rows_1024"] > b["tables/D1024/rows_1025"]                       # tickets + sliced tables: small batches only
    for tag in mk.LENGTHS:
        for t in (0, 1):
            assert len({b[f"workspace_for/D260/{tag}/train{t}/prec{p}"] for p in (0, 1, 2)}) == 1, (tag, t)
            assert b[f"workspace_for/D260/{tag}/train{t}/prec3"] == b[f"workspace/D260/{tag}/train{t}"]
    for D in mk.DIMS:
        for n in mk.PLANES:
            assert (b[f"wplanes/D{D}/np{n}"] > 0) == (D % 256 == 0 and n in (2, 3)), (D, n)
