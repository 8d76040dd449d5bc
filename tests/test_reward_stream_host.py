"""CPU: what the streaming DSN reward (csrc/reward_stream.hip) promises without a device -- the recipe conditions of
tests/reward_stream_cases.py on the oracle alone, the workspace query (pure host arithmetic: O(E x n_rows), never O(T^2)), the refusals of
sumk_dsn_reward_stream (they come before anything touches a device: made-up pointers, refused calls only) and the exported symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import reward_stream_cases as RS
from conftest import ROOT

LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")
GIB = 1 << 30


@pytest.mark.parametrize("name", RS.NEW_FAMILIES)
def test_recipes_keep_both_reward_terms_visible(name):
    """Every compared case has R_rep >= 0.2 in float64, and the family's yardstick (largest |fp32 oracle - float64 oracle|) is a rounding
    error, not zero and not a cancellation: 0 < yardstick <= 1e-6.  (tests/test_oracle.py says the same of the families of recipes.py.)"""
    calls, refs, yard = RS.family(name)
    assert calls and 0 < yard <= 1e-6, (name, yard)
    n = 0
    for call, (t64, r32) in zip(calls, refs):
        picked = np.array([[call["acts"][e, o:o + T].any() for o, T in zip(np.concatenate([[0], np.cumsum(call["lens"])]), call["lens"])]
                           for e in range(call["acts"].shape[0])])
        fin = np.isfinite(t64[:, :, 2])
        assert (t64[:, :, 1][picked & fin] >= 0.2).all(), (call["id"], t64[:, :, 1])
        assert (t64[~picked] == 0).all() and (r32[~picked] == 0).all(), call["id"]
        for (e, s), what in call.get("expect", {}).items():
            assert (what == "no_pick") == (not picked[e, s]), (call["id"], e, s, what)
        n += int((picked & fin).sum())
    assert n > 0
    if name == "zero_norm":
        assert all(np.array_equal(np.isnan(t64[:, :, 2]), RS.ZERO_NORM_NAN) for t64, _ in refs)
    if name == "tile_edges":
        assert {(c["thre"], c["expect"][(0, 0)]) for c in calls if c["id"].endswith("picks63_84_far0")} == \
            {(0, "beyond_thre"), (1, "beyond_thre"), (20, "beyond_thre"), (21, "within_thre")}
    if name == "chunks":
        assert sorted({c["acts"].shape[0] for c in calls}) == sorted(RS.CHUNK_E)


# ------------------------------------------------------------------------------------------------ the C entries, without a device
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(LIB)
    i32p = C.POINTER(C.c_int32)
    for name in ("sumk_dsn_reward_stream_workspace_bytes", "sumk_dsn_reward_workspace_bytes"):
        getattr(lib, name).restype = C.c_size_t
        getattr(lib, name).argtypes = [C.c_int32, C.c_int32, i32p, C.c_int32]
    lib.sumk_dsn_reward_stream_plan.restype = C.c_int32
    lib.sumk_dsn_reward_stream_plan.argtypes = [C.c_int32, i32p]
    lib.sumk_dsn_reward_stream.restype = C.c_int
    lib.sumk_dsn_reward_stream.argtypes = [C.c_void_p, C.c_int32, C.c_int32, i32p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.sumk_last_error.restype = C.c_char_p
    return lib


def _off(lens):
    return (C.c_int32 * (len(lens) + 1))(*np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist())


def test_workspace_is_linear_in_the_rows(lib):
    q = lambda D, lens, E: lib.sumk_dsn_reward_stream_workspace_bytes(D, len(lens), _off(lens), E)
    gram = lambda D, lens, E: lib.sumk_dsn_reward_workspace_bytes(D, len(lens), _off(lens), E)
    # the library's long-video limit: under 1 GiB where the Gram path asks for more than 4 TB
    big = q(1024, [1 << 20], 5)
    assert 0 < big < GIB, big
    assert gram(1024, [1 << 20], 5) > 4 * 10 ** 12
    # it holds at least the partials: (min, cos sum, far count) x 4 bytes per (episode, row, split) for the 8 splits it is sized for
    assert big >= 3 * 4 * 5 * 8 * (1 << 20)
    # linear in T (within alignment slack), no T^2 term
    a, b = q(1024, [1 << 16], 5), q(1024, [1 << 17], 5)
    assert abs(b - 2 * a) <= 16 * 256, (a, b)
    # episodes past one chunk add their pick bits only: the partials hold one chunk
    assert q(1024, [1 << 16], RS.EC) < q(1024, [1 << 16], 4 * RS.EC) < q(1024, [1 << 16], RS.EC) + 4 * RS.EC * (1 << 16) // 8 + 4096
    assert q(1024, [300], 5) == q(8, [300], 5)                                    # D decides nothing but eligibility
    assert 0 < q(8, [1], 1) and 0 < q(36, [60, 1, 193, 130, 64], 17)
    for bad in ((6, [130], 5), (0, [130], 5), (1024, [(1 << 20) + 1], 5), (1024, [130, 0], 5), (1024, [130], 0), (1024, [], 5)):
        assert q(*bad) == 0, bad
        assert b"dsn_reward_stream" in lib.sumk_last_error(), bad
    assert lib.sumk_dsn_reward_stream_workspace_bytes(1024, 1, None, 5) == 0


def test_plan_is_one_round_of_workgroups_capped_at_eight(lib):
    plan = lambda lens: lib.sumk_dsn_reward_stream_plan(len(lens), _off(lens))
    assert plan([193]) == 8 and plan([1]) == 8 and plan([700]) == 8               # few strips: the cap (a video takes at most its tiles)
    assert plan([16384]) == 4 and plan([65536]) == 1 and plan([1 << 20]) == 1     # 256 strips x 4 = 1024 resident workgroups
    assert plan([3600] * 8) == 2
    assert lib.sumk_dsn_reward_stream_plan(0, _off([])) == 0 and lib.sumk_dsn_reward_stream_plan(1, None) == 0


def test_refusals_launch_nothing(lib):
    """Every refused call returns the library's status code with a message before it touches its pointers: these are made up."""
    fake = lambda k: C.c_void_p(0x1000 * (k + 1))
    need = lib.sumk_dsn_reward_stream_workspace_bytes(64, 1, _off([130]), 5)
    assert need > 0

    def call(lens=(130,), D=64, E=5, col_split=0, ws_bytes=need, x=fake(0), off_dev=fake(1), acts=fake(2), reward=fake(3), ws=fake(4), off_host=True):
        lens = list(lens)
        return lib.sumk_dsn_reward_stream(x, D, len(lens), _off(lens) if off_host else None, off_dev, acts, E, 0, 20, col_split, reward, ws, ws_bytes,
                                          None)

    bad = [("D=6", dict(D=6), -1, "D=6"), ("col_split=9", dict(col_split=9), -1, "col_split=9"), ("col_split=-1", dict(col_split=-1), -1, "col_split"),
           ("empty batch", dict(lens=[]), -1, "empty batch"), ("no episodes", dict(E=0), -1, "empty batch"),
           ("an empty video", dict(lens=[130, 0]), -1, "frames"), ("T past the limit", dict(lens=[(1 << 20) + 1], ws_bytes=1 << 40), -1, "frames"),
           ("null x", dict(x=None), -1, "null"), ("null actions", dict(acts=None), -1, "null"), ("null reward", dict(reward=None), -1, "null"),
           ("null workspace", dict(ws=None), -1, "null"), ("null offsets", dict(off_dev=None), -1, "null"),
           ("null host offsets", dict(off_host=False), -1, "empty batch"), ("misaligned x", dict(x=C.c_void_p(0x1004)), -1, "aligned"),
           ("short workspace", dict(ws_bytes=need - 1), -2, "workspace")]
    for tag, kw, code, word in bad:
        rc = call(**kw)
        msg = lib.sumk_last_error().decode()
        assert rc == code and "dsn_reward_stream" in msg and word in msg, (tag, rc, msg)


def test_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "sumk.h")).read()
    for name in ("sumk_dsn_reward_stream", "sumk_dsn_reward_stream_workspace_bytes"):
        assert name + "(" in header and hasattr(lib, name), name
    assert "SUMK_REWARD_STREAM_EC %d" % RS.EC in header


def test_python_layer_refuses_an_unknown_path():
    from summarizer_amd import kernels
    from summarizer_amd._lib import SumkError
    assert kernels.REWARD_PATHS == ("gram", "stream") and kernels.REWARD_STREAM_EC == RS.EC
    with pytest.raises(SumkError, match="path"):
        kernels._reward_path("banded")
