"""CPU: the positional entry points of csrc/posembed.hip refuse bad arguments on the host, before anything is launched -- so these
answers need no GPU."""
import ctypes as C
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(LIB)
    lib.sumk_last_error.restype = C.c_char_p
    i32, vp, hp = C.c_int32, C.c_void_p, C.POINTER(C.c_int32)
    lib.sumk_pos_add_packed.argtypes = [vp, i32, i32, hp, vp, vp, i32, vp, vp, vp, i32, vp]
    lib.sumk_pos_table_grad.argtypes = [vp, i32, i32, hp, vp, vp, i32, vp]
    return lib


def test_pos_entry_points_refuse_bad_arguments_on_the_host(lib):
    off = (C.c_int32 * 4)(0, 5, 70, 71)           # videos of 5, 65 and 1 frames
    p = 0x1000                                    # (never dereferenced: every call below is refused before a launch)
    add = lambda D, rows, o32=p, o16=None, pl=None, npl=0, n_seq=3, o=off: lib.sumk_pos_add_packed(p, D, n_seq, o, p, p, rows, o32, o16, pl, npl, None)
    assert add(64, 64) != 0 and b"max_length" in lib.sumk_last_error()             # a video one frame longer than the table
    assert add(6, 65) != 0                                                         # D % 4
    assert add(24, 65, None, None, p, 2) != 0 and add(64, 65, None, None, p, 4) != 0      # planes: D % 16, 2 or 3 planes
    assert add(64, 65, None) != 0                                                  # no output asked for
    assert add(64, 65, p + 4) != 0                                                 # alignment
    assert add(64, 65, o=(C.c_int32 * 4)(0, 5, 5, 71)) != 0                        # an empty video
    assert add(64, 65, n_seq=0) != 0
    assert lib.sumk_pos_table_grad(p, 64, 3, off, p, p, 64, None) != 0 and b"max_length" in lib.sumk_last_error()
    assert lib.sumk_pos_table_grad(p, 6, 3, off, p, p, 65, None) != 0
    assert lib.sumk_pos_table_grad(p, 64, 3, off, p, None, 65, None) != 0
