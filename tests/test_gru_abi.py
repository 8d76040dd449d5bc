"""CPU: the persistent BiGRU layer is part of the C ABI -- include/sumk.h declares its four entry points, the cross-compiled
libsumk.so exports them and the ctypes binding table carries them; its size query is host arithmetic and refuses shapes outside
the kernel's domain.  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sumk.h")
LIB = os.path.join(ROOT, "summarizer_amd", "libsumk.so")
NEW = ["sumk_bigru_workspace_bytes", "sumk_bigru_layer_forward", "sumk_bigru_layer_backward", "sumk_bigru_check"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(LIB)


def test_header_declares_the_bigru_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert "sumk_gru_layer_weights" in src and "sumk_gru_layer_grads" in src
    # the step path stays in the ABI: it serves H > 256
    assert re.search(r"\bsumk_gru_cell_forward\s*\(", src) and re.search(r"\bsumk_gru_cell_backward\s*\(", src)


def test_library_exports_the_bigru_entry_points(lib):
    missing = [n for n in NEW if not hasattr(lib, n)]
    assert not missing, missing


def test_binding_table_carries_the_bigru_entry_points():
    from summarizer_amd import _lib
    for name in NEW:
        assert name in _lib._SIGS, name
    assert len(_lib._SIGS["sumk_bigru_layer_forward"][1]) == 13 and len(_lib._SIGS["sumk_bigru_layer_backward"][1]) == 15
    w = _lib.GruLayerWeights()
    assert C.sizeof(w) == 8 * C.sizeof(C.c_void_p) and C.sizeof(_lib.GruLayerGrads()) == 8 * C.sizeof(C.c_void_p)


def test_workspace_query_is_host_arithmetic_and_knows_the_domain(lib):
    f = lib.sumk_bigru_workspace_bytes
    f.restype = C.c_size_t
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    off = np.array([0, 300, 301, 550], dtype=np.int32)
    p = off.ctypes.data_as(C.POINTER(C.c_int32))
    R = 550
    inf, trn = f(1024, 256, 3, p, 0), f(1024, 256, 3, p, 1)
    assert inf >= R * 6 * 256 * 4                                   # the projection's output at least
    assert trn >= inf + R * (8 + 2 + 6 + 2) * 256 * 4               # + r, z, n, Gh_n, h_prev, dGx and the n block of dGh
    for H in (4, 16, 40, 200, 252):
        assert 0 < f(64, H, 3, p, 0) < f(64, H, 3, p, 1), H
    for bad in ((1024, 260), (1024, 0), (1024, 18), (1022, 256), (0, 256)):
        assert f(bad[0], bad[1], 3, p, 1) == 0, bad
    off_bad = np.array([0, 5, 5], dtype=np.int32)                   # an empty video
    assert f(64, 16, 2, off_bad.ctypes.data_as(C.POINTER(C.c_int32)), 0) == 0
