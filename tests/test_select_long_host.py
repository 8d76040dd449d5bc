"""CPU: the host side of the long-video evaluation tail (csrc/evallong.hip) -- the workspace arithmetic of sumk_eval_device_select_long
and its refusals, the limits of include/sumk.h against their mirrors in utils/eval_native.py, `select_long_refusal` in words, and the
`tail` argument of `Summarizer`.  No kernel runs here."""
import os
import re

import pytest

from conftest import ROOT


def _macros():
    src = open(os.path.join(ROOT, "include", "sumk.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (SUMK_[A-Z_]+) (\d+)$", src, flags=re.M)}


def _up(b):
    return (b + 255) // 256 * 256


def _formula(n_videos, S, cap, m):
    """The layout include/sumk.h documents, per video and each part rounded up to 256 bytes."""
    bits = _up(S * ((cap + 1 + 63) // 64) * 8)
    rows = _up(2 * (cap + 1) * 4)
    items = _up((5 * S + 9) * 4)
    counts = _up(m["SUMK_SELECT_LONG_FRAME_CHUNKS"] * (2 * m["SUMK_SELECT_MAX_USERS"] + 1) * 4)
    return n_videos * (bits + rows + items + counts)


def test_workspace_bytes_equal_the_documented_formula():
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    lib, m = _lib.load(), _macros()
    chunk = m["SUMK_SELECT_LONG_CHUNK"]
    for n_videos in (1, 3, 63):
        for S in (1, 2, 64, 65, 1024):
            for cap in (0, 1, 62, 63, 64, chunk - 1, chunk, chunk + 1, 8191, 8192, 147456, 1 << 24):
                want = _formula(n_videos, S, cap, m)
                assert lib.sumk_eval_device_select_long_workspace_bytes(n_videos, S, cap) == want, (n_videos, S, cap)
                assert eval_native.select_long_workspace_bytes(n_videos, S, cap) == want, (n_videos, S, cap)
    # the README's own example: one video, 1024 segments, a budget of 147 456 frames -- 18.0 MiB of improvement bits
    assert 1024 * 2305 * 8 < lib.sumk_eval_device_select_long_workspace_bytes(1, 1024, 147456) < 1024 * 2305 * 8 + (2 << 20)


def test_workspace_bytes_refuse_what_the_call_refuses():
    from summarizer_amd import _lib
    lib = _lib.load()
    assert lib.sumk_eval_device_select_long_workspace_bytes(1, 1, 0) > 0 and lib.sumk_eval_device_select_long_workspace_bytes(1, 1024, 1 << 24) > 0
    for bad in ((1, 0, 100), (1, 1025, 100), (1, 10, -1), (1, 10, (1 << 24) + 1), (0, 10, 100), (-1, 10, 100)):
        assert lib.sumk_eval_device_select_long_workspace_bytes(*bad) == 0, bad


def test_header_limits_equal_the_python_constants():
    from summarizer_amd import kernels
    from summarizer_amd.utils import eval_native
    m = _macros()
    assert m["SUMK_SEGMENTS_LONG_MAX_PICKS"] == eval_native.SEGMENTS_LONG_MAX_PICKS == kernels.KTS_BANDED_MAX_STEPS      # the cap of sumk_kts_banded
    assert m["SUMK_SEGMENTS_LONG_MAX_FRAMES"] == eval_native.SEGMENTS_LONG_MAX_FRAMES == 1 << 24
    assert m["SUMK_SELECT_LONG_MAX_CAPACITY"] == eval_native.SELECT_LONG_MAX_CAPACITY == 1 << 24
    assert m["SUMK_SELECT_LONG_CHUNK"] == eval_native.SELECT_LONG_CHUNK and m["SUMK_SELECT_LONG_CHUNK"] % 64 == 0
    assert m["SUMK_SELECT_LONG_FRAME_CHUNKS"] == eval_native.SELECT_LONG_FRAME_CHUNKS
    # the limits the two selections share are untouched
    assert (m["SUMK_SELECT_MAX_SEGS"], m["SUMK_SELECT_MAX_CAPACITY"], m["SUMK_SELECT_MAX_USERS"]) == (1024, 8191, 32)
    assert (eval_native.SELECT_MAX_SEGS, eval_native.SELECT_MAX_CAPACITY, eval_native.SELECT_MAX_USERS) == (1024, 8191, 32)


def test_select_long_refusal_names_the_limit():
    from summarizer_amd.utils.eval_native import select_long_refusal, select_refusal
    assert select_long_refusal(1024, 983040, 20, 0.15) is None                       # 65 536 steps x 15 frames: a budget of 147 456
    assert "budget of 147456" in select_refusal(1024, 983040, 20, 0.15)              # what the one-workgroup call says to the same video
    assert select_long_refusal(1, 1, 0, 0.15) is None and select_long_refusal(41, 61500, 0, 0.15) is None
    assert select_long_refusal(1024, 1 << 24, 32, 1.0) is None                       # every limit at once
    assert "0 segments (1 .. 1024)" in select_long_refusal(0, 100, 0, 0.15)
    assert "1025 segments (1 .. 1024)" in select_long_refusal(1025, 100, 0, 0.15)
    assert "33 annotators (at most 32)" in select_long_refusal(10, 100, 33, 0.15)
    assert f"{(1 << 24) + 1} frames (1 .. {1 << 24})" in select_long_refusal(10, (1 << 24) + 1, 0, 0.15)
    assert "0 frames" in select_long_refusal(10, 0, 0, 0.15)
    why = select_long_refusal(10, 1 << 24, 0, 1.5)
    assert "budget of 25165824 frames" in why and f"(0 .. {1 << 24})" in why
    assert "budget of -" in select_long_refusal(10, 100, 0, -0.5)


class _Scorer:
    def score_packed(self, packed, lens):
        raise AssertionError("nothing is scored in these tests")


def test_summarizer_tail_argument_is_checked():
    import summarizer_amd
    from summarizer_amd._lib import SumkError
    with pytest.raises(SumkError, match="device=True"):
        summarizer_amd.Summarizer(_Scorer(), tail="long", device=False)
    with pytest.raises(SumkError, match="device=True"):
        summarizer_amd.Summarizer(_Scorer(), tail="long")
    with pytest.raises(KeyError, match="Unknown tail"):
        summarizer_amd.Summarizer(_Scorer(), tail="chip", device=True)
    assert summarizer_amd.Summarizer(_Scorer()).tail == "block" and summarizer_amd.Summarizer(_Scorer(), device=True).tail == "block"
    assert summarizer_amd.Summarizer(_Scorer(), device=True, tail="long", kts="banded").tail == "long"


def test_summarizer_long_tail_refuses_before_anything_is_enqueued():
    """The checks of tail="long" read lengths only: they run -- and refuse -- without a GPU, before the scorer is called."""
    import numpy as np
    import summarizer_amd
    from summarizer_amd._lib import SumkError
    s = summarizer_amd.Summarizer(_Scorer(), device=True, tail="long", kts="banded", max_ncp=40, lmax=512)
    with pytest.raises(SumkError, match="1048577 picks"):
        s._check_long_limits([1048577], [None], [None])
    with pytest.raises(SumkError, match=rf"{(1 << 24) + 1} frames"):
        s._check_long_limits([100], [None], [(1 << 24) + 1])
    with pytest.raises(SumkError, match="ascend"):
        s._check_long_limits([100], [np.arange(100)[::-1].copy()], [100])
    with pytest.raises(SumkError, match="1025 segments"):
        summarizer_amd.Summarizer(_Scorer(), device=True, tail="long", max_ncp=1024)._check_long_limits([5000], [None], [None])
    with pytest.raises(SumkError, match="max_workspace_bytes=1000"):
        summarizer_amd.Summarizer(_Scorer(), device=True, tail="long", max_ncp=40, max_workspace_bytes=1000)._check_long_limits([4100], [None], [61500])
    # 1024 segments at a budget of 2^24 x 0.9 frames: 1.9 GiB of improvement bits per video, five of them pass the default of 8 GiB
    with pytest.raises(SumkError, match="max_workspace_bytes="):
        summarizer_amd.Summarizer(_Scorer(), device=True, tail="long", proportion=0.9, max_ncp=1023)._check_long_limits([5000] * 5, [None] * 5, [1 << 24] * 5)
    nf, pk = s._check_long_limits([4100, 300], [15 * np.arange(4100), None], [61500, None])
    assert nf == [61500, 300] and pk[0].dtype == np.int32 and pk[1] is None
