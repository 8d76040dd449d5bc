"""GPU: dataset records from raw annotations (csrc/annotate.hip: sumk_annotate, sumk_annotate_gtsummary; summarizer_amd/utils/annotate.py:
AnnotateChain / annotate_batch / build_records and the command line).

The reference throughout is tests/annotate_ref.py (plain numpy, float32 operation for operation; the summaries through the host
`utils.eval.generate_summary`) and, for the change points, tests/kts_ref.py.  Every comparison is `assert_array_equal`: no tolerance
appears anywhere in this file.  The references are computed once per module and shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import annotate_ref as A
import kts_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
PROTOCOLS = ("scores", "summaries")


def _dev():
    return torch.device("cuda:0")


def _poisoned(numel, dtype, dev):
    t = torch.empty(max(int(numel), 1), dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(255)
    return t


def _picks(n_picks, n_frames, short):
    """n_picks ascending positions, the last one `short` frames before the end of the video."""
    if n_picks == 1:
        return np.array([max(0, n_frames - 1 - short)], np.int32)
    return np.floor(np.linspace(0, n_frames - 1 - short, n_picks)).astype(np.int32)


def _video(name, U, n_frames, n_picks, lengths, n_pad, seed, short=0, constant=False):
    assert sum(lengths) == n_frames
    cps, nfps = A.segments_of_lengths(lengths, n_pad)
    v = {"name": name, "n_frames": n_frames, "picks": _picks(n_picks, n_frames, short), "cps": cps, "nfps": nfps,
         "scores": np.full((U, n_frames), 3, F32) if constant else A.block_grades(U, n_frames, seed),
         "summaries": np.full((U, n_frames), 2, F32) if constant else A.block_selections(U, n_frames, seed + 1)}
    return v


# U in {1, 2, 20, 32}; n_frames in {1, 17, 129, 300, 4494}; segment lengths 1, 7, 8, 9, 128, 129, 257 inside one video (the pairwise tree changes
# shape at 8 and at 128); empty pad segments; n_picks in {1, 2, 300} with the last pick short of n_frames - 1; grades held over 30 frames; one
# all-equal video
LONG = [1, 7, 8, 9, 128, 129, 257, 30, 60, 90, 120, 150, 180, 210, 240, 270, 300, 330, 360, 390, 420, 450, 355]
VIDEOS = [
    _video("one-frame", 1, 1, 1, [1], 0, 11),
    _video("two-annotators", 2, 17, 2, [1, 7, 9], 1, 12, short=3),
    _video("129-frames", 20, 129, 2, [128, 1], 2, 13, short=1),
    _video("32-annotators", 32, 300, 2, [8, 7, 9, 129, 147], 0, 14, short=40),
    _video("tvsum-shaped", 20, 4494, 300, LONG, 3, 15, short=8),
    _video("all-equal", 3, 300, 1, [100, 100, 100], 0, 16, short=299, constant=True),
]
assert sum(LONG) == 4494 and int(VIDEOS[4]["picks"][-1]) == 4485
RAGGED = [VIDEOS[3], VIDEOS[1], VIDEOS[4]]          # the whole-chain batch: three such videos of different lengths


@functools.lru_cache(maxsize=None)
def _frame_level(i, protocol):
    v = VIDEOS[i]
    return A.scores_frame_level(v["scores"], v["picks"], v["cps"]) if protocol == "scores" else A.summaries_frame_level(v["summaries"], v["picks"])


@functools.lru_cache(maxsize=None)
def _record(name, protocol, method):
    v = next(x for x in VIDEOS if x["name"] == name)
    return A.record(v[protocol], v["picks"], v["n_frames"], v["cps"], v["nfps"], protocol, (1, 5), 0.15, method)


def _upload(vids, protocol, dev):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return ([up(v[protocol]) for v in vids], [up(v["picks"]) for v in vids], [v["n_frames"] for v in vids],
            [(up(v["cps"]), up(v["nfps"])) for v in vids])


# ------------------------------------------------------------------------------------------------ 1. the C entry
def _raw_call(vids, protocol, lo=1.0, hi=5.0, gap=3, override=None, null=(), dev_override=None):
    """sumk_annotate on buffers of the test's own, all filled with 0xFF bytes first, the videos' ranges `gap` elements apart in every output.
    override: {video: {field: value}} on the host AND device copy of the descriptors; dev_override: on the device copy alone; null: names
    of the call's own pointers to pass as NULL."""
    from summarizer_amd import _lib
    lib, dev, n = _lib.load(), _dev(), len(vids)
    annos, picks, _, segs = _upload(vids, protocol, dev)
    d = (_lib.AnnotateVideo * n)()
    at = {"user": gap, "frame": gap, "pick": gap, "seg": gap}
    where = []
    for i, v in enumerate(vids):
        e, (U, F), NP, S = d[i], v[protocol].shape, len(v["picks"]), len(v["cps"])
        e.anno, e.picks, e.cps = annos[i].data_ptr(), picks[i].data_ptr(), segs[i][0].data_ptr()
        e.n_users, e.n_frames, e.n_picks, e.n_segs, e.summary_len = U, F, NP, S, int(v["nfps"].sum())
        e.user0, e.frame0, e.pick0, e.seg0, e.gtsum0 = at["user"], at["frame"], at["pick"], at["seg"], at["frame"]
        where.append(dict(user=(at["user"], U * F), frame=(at["frame"], F), pick=(at["pick"], NP), seg=(at["seg"], U * S)))
        at["user"] += U * F + gap; at["frame"] += F + gap; at["pick"] += NP + gap; at["seg"] += U * S + gap
        for k, val in (override or {}).get(i, {}).items():
            setattr(e, k, val)
    on_dev = (_lib.AnnotateVideo * n).from_buffer_copy(bytes(d))
    for i, fields in (dev_override or {}).items():
        for k, val in fields.items():
            setattr(on_dev[i], k, val)
    d_dev = torch.frombuffer(bytearray(bytes(on_dev)), dtype=torch.uint8).to(dev)
    bufs = {k: _poisoned(at[k], torch.float32, dev) for k in at}
    bufs["gtsummary"] = _poisoned(at["pick"], torch.float32, dev)
    ptr = lambda name, t: None if name in null else t.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.sumk_annotate(ptr("videos_dev", d_dev), None if "videos_host" in null else C.cast(d, C.c_void_p), n, A_PROTOCOL[protocol], lo, hi,
                           ptr("user", bufs["user"]), at["user"], ptr("frame", bufs["frame"]), at["frame"], ptr("pick", bufs["pick"]), at["pick"],
                           ptr("seg", bufs["seg"]), at["seg"], st)
    err = lib.sumk_last_error().decode(errors="replace")
    torch.cuda.synchronize(dev)
    raw = {k: t.cpu().numpy() for k, t in bufs.items()}
    return dict(rc=rc, error=err, raw=raw, where=where, descr=d, descr_dev=d_dev, bufs=bufs, at=at, keep=(annos, picks, segs))


A_PROTOCOL = {"scores": 0, "summaries": 1}
POISON = np.frombuffer(b"\xff\xff\xff\xff", dtype=np.uint32)[0]


def _untouched(a):
    return bool(np.all(a.view(np.uint32) == POISON))


def _cut(out, i, key):
    lo, n = out["where"][i][key]
    return out["raw"][key][lo:lo + n]


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_c_entry_equals_the_specification(protocol):
    out = _raw_call(VIDEOS, protocol)
    assert out["rc"] == 0, out["error"]
    for i, v in enumerate(VIDEOS):
        want, (U, F), S = _frame_level(i, protocol), v[protocol].shape, len(v["cps"])
        user = _cut(out, i, "user").reshape(U, F)
        assert_array_equal(user, want["user_scores" if protocol == "scores" else "user_summary"], err_msg=v["name"])
        assert_array_equal(_cut(out, i, "frame"), want["consensus"], err_msg=v["name"])
        assert_array_equal(_cut(out, i, "pick"), want["gtscore"], err_msg=v["name"])
        if protocol == "scores":
            assert_array_equal(_cut(out, i, "seg").reshape(U, S), want["seg_means"], err_msg=v["name"])
    if protocol == "scores":
        assert_array_equal(_cut(out, 5, "pick"), np.zeros(1, F32))                      # the all-equal video: max == min
        assert not np.any(_frame_level(4, protocol)["seg_means"][:, -3:])              # the pad segments: mean 0
        means = _frame_level(4, protocol)["seg_means"]
        assert all(len(set(row[:-3].tolist())) < len(row) - 3 for row in means)             # block grades: equal segment means exist
    # what lies between the videos' ranges stays as it was
    for key, buf in out["raw"].items():
        outside = np.ones(buf.shape[0], bool)
        if key in ("user", "frame", "pick") or (key == "seg" and protocol == "scores"):
            for w in out["where"]:
                outside[w[key][0]:w[key][0] + w[key][1]] = False
        assert _untouched(buf[outside]), key


def test_c_entry_accepts_the_most_videos_one_call_takes():
    """65535 videos (the limit) of 257 frames: 2 x 65535 blocks in the frame pass, far inside one launch, so the call is accepted.  Every
    descriptor is the SAME video on the same output ranges (real buffers; every block writes the values its twins write), so the outputs
    are that video's, and nothing outside its ranges is touched."""
    v = _video("257-frames", 3, 257, 2, [128, 129], 0, 17, short=5)
    n = 65535
    out = _raw_call([v], "scores")
    assert out["rc"] == 0, out["error"]
    first = {k: a.copy() for k, a in out["raw"].items()}
    from summarizer_amd import _lib
    lib, dev = _lib.load(), _dev()
    many = (_lib.AnnotateVideo * n)(*([out["descr"][0]] * n))
    many_dev = torch.frombuffer(bytearray(bytes(many)), dtype=torch.uint8).to(dev)
    b, at = out["bufs"], out["at"]
    for t in b.values():
        t.view(torch.uint8).fill_(255)
    rc = lib.sumk_annotate(many_dev.data_ptr(), C.cast(many, C.c_void_p), n, 0, 1.0, 5.0, b["user"].data_ptr(), at["user"], b["frame"].data_ptr(), at["frame"],
                           b["pick"].data_ptr(), at["pick"], b["seg"].data_ptr(), at["seg"], C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, lib.sumk_last_error()
    torch.cuda.synchronize(dev)
    want = A.scores_frame_level(v["scores"], v["picks"], v["cps"])
    assert_array_equal(_cut(out, 0, "user").reshape(3, 257), want["user_scores"])
    for key in ("user", "frame", "pick", "seg"):
        assert_array_equal(b[key].cpu().numpy().view(np.uint32), first[key].view(np.uint32), err_msg=key)


def test_gtsummary_gathers_the_frame_summary_at_the_picks():
    from summarizer_amd import _lib
    lib, dev = _lib.load(), _dev()
    out = _raw_call(VIDEOS, "summaries")
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 2, size=out["at"]["frame"]).astype(F32)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.sumk_annotate_gtsummary(out["descr_dev"].data_ptr(), C.cast(out["descr"], C.c_void_p), len(VIDEOS), torch.from_numpy(frames).to(dev).data_ptr(),
                                     out["at"]["frame"], out["bufs"]["gtsummary"].data_ptr(), out["at"]["pick"], st)
    assert rc == 0, lib.sumk_last_error()
    torch.cuda.synchronize(dev)
    got = out["bufs"]["gtsummary"].cpu().numpy()
    outside = np.ones(got.shape[0], bool)
    for v, w in zip(VIDEOS, out["where"]):
        assert_array_equal(got[w["pick"][0]:w["pick"][0] + w["pick"][1]], frames[w["frame"][0] + v["picks"].astype(np.int64)])
        outside[w["pick"][0]:w["pick"][0] + w["pick"][1]] = False
    assert _untouched(got[outside])


def test_bad_device_descriptors_stay_in_bounds():
    """What the entry point cannot see: picks and change points outside the video are clamped, a device descriptor past the limits is
    skipped -- the other video's results and everything outside the ranges are unchanged."""
    vids = [dict(VIDEOS[1]), dict(VIDEOS[2])]
    vids[0]["picks"] = np.array([-5, 4000], np.int32)
    vids[0]["cps"] = np.array([[-3, 0], [1, 7], [8, 90], [17, 16]], np.int32)
    out = _raw_call(vids, "scores", dev_override={1: {"n_users": 33}})
    assert out["rc"] == 0, out["error"]
    want = A.scores_frame_level(vids[0]["scores"], np.array([0, 16]), np.array([[0, 0], [1, 7], [8, 16], [17, 16]]))
    assert_array_equal(_cut(out, 0, "pick"), want["gtscore"])
    assert_array_equal(_cut(out, 0, "seg").reshape(2, 4), want["seg_means"])
    for key in ("user", "frame", "pick", "seg"):
        assert _untouched(_cut(out, 1, key)), key


# ------------------------------------------------------------------------------------------------ 2. refusals
REFUSALS = {
    "33 annotators": dict(override={0: {"n_users": 33}}),
    "reserved field set": dict(override={1: {"reserved": 7}}),
    "no annotators": dict(override={0: {"n_users": 0}}),
    "4096 picks": dict(override={0: {"n_picks": 4096}}),
    "no picks": dict(override={0: {"n_picks": 0}}),
    "1025 segments": dict(override={0: {"n_segs": 1025}}),
    "no segments": dict(override={0: {"n_segs": 0}}),
    "frames past 2^24": dict(override={0: {"n_frames": (1 << 24) + 1, "summary_len": (1 << 24) + 1}}),
    "hi == lo": dict(lo=2.0, hi=2.0),
    "hi < lo": dict(lo=5.0, hi=1.0),
    "nan bound": dict(lo=float("nan"), hi=5.0),
    "infinite bound": dict(lo=1.0, hi=float("inf")),
    "null annotations": dict(override={1: {"anno": None}}),
    "null picks": dict(override={1: {"picks": None}}),
    "null change points": dict(override={1: {"cps": None}}),
    "null output": dict(null=("user",)),
    "null consensus": dict(null=("frame",)),
    "null gtscore": dict(null=("pick",)),
    "null segment means": dict(null=("seg",)),
    "null descriptors": dict(null=("videos_dev",)),
    "null host descriptors": dict(null=("videos_host",)),
    "segments short of the frames": dict(override={1: {"summary_len": 128}}),
    "segments past the frames": dict(override={0: {"summary_len": 18}}),
    "rows outside the output": dict(override={1: {"user0": 1 << 40}}),
    "negative offset": dict(override={0: {"frame0": -1}}),
    "picks outside the output": dict(override={1: {"pick0": 10 ** 6}}),
    "segment means outside the output": dict(override={1: {"seg0": 10 ** 6}}),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_c_entry_refuses_and_launches_nothing(name):
    out = _raw_call([VIDEOS[1], VIDEOS[2]], "scores", **REFUSALS[name])
    assert out["rc"] == -1 and out["error"], name
    for key, buf in out["raw"].items():
        assert _untouched(buf), (name, key)


def test_c_entry_refuses_protocol_and_gtsummary_arguments():
    from summarizer_amd import _lib
    lib, dev = _lib.load(), _dev()
    out = _raw_call([VIDEOS[1]], "scores")
    d, dd, b, at = out["descr"], out["descr_dev"], out["bufs"], out["at"]
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for t in b.values():
        t.view(torch.uint8).fill_(255)
    args = lambda protocol: (dd.data_ptr(), C.cast(d, C.c_void_p), 1, protocol, 1.0, 5.0, b["user"].data_ptr(), at["user"], b["frame"].data_ptr(), at["frame"],
                             b["pick"].data_ptr(), at["pick"], b["seg"].data_ptr(), at["seg"], st)
    assert lib.sumk_annotate(*args(2)) == -1 and lib.sumk_annotate(*args(-1)) == -1
    assert lib.sumk_annotate(dd.data_ptr(), C.cast(d, C.c_void_p), -1, *args(0)[3:]) == -1
    assert lib.sumk_annotate(None, None, 0, 0, 1.0, 5.0, None, 0, None, 0, None, 0, None, 0, st) == 0          # an empty batch is fine
    g = lambda fs, total, out_p, picks: lib.sumk_annotate_gtsummary(dd.data_ptr(), C.cast(d, C.c_void_p), 1, fs, total, out_p, picks, st)
    assert g(None, at["frame"], b["gtsummary"].data_ptr(), at["pick"]) == -1
    assert g(b["frame"].data_ptr(), at["frame"], None, at["pick"]) == -1
    assert g(b["frame"].data_ptr(), 10, b["gtsummary"].data_ptr(), at["pick"]) == -1                           # the video's frames lie outside
    assert g(b["frame"].data_ptr(), at["frame"], b["gtsummary"].data_ptr(), 1) == -1
    d[0].n_picks = 4096
    assert g(b["frame"].data_ptr(), at["frame"], b["gtsummary"].data_ptr(), at["pick"]) == -1
    torch.cuda.synchronize(dev)
    for key, t in b.items():
        assert _untouched(t.cpu().numpy()), key


# ------------------------------------------------------------------------------------------------ 3. the whole chain
def _check_chain(res, vids, protocol, method):
    for r, v in zip(res, vids):
        want = _record(v["name"], protocol, method)
        assert_array_equal(r["status"], np.zeros_like(r["status"]), err_msg=v["name"])
        for key in ("user_scores", "user_summary", "gtscore", "gtsummary", "consensus", "gt_seg_means", "gt_frame_summary", "gt_selected"):
            assert_array_equal(r[key], want[key], err_msg=f"{v['name']} {key}")
            assert r[key].dtype == want[key].dtype, key
        if protocol == "scores":
            assert_array_equal(r["seg_means"], want["seg_means"], err_msg=v["name"])
            assert_array_equal(r["user_selected"], want["user_selected"], err_msg=v["name"])


@pytest.mark.parametrize("method", ["knapsack", "rank"])
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_chain_equals_the_specification(protocol, method):
    from summarizer_amd.utils import annotate as M
    dev = _dev()
    res = M.annotate_batch(*_upload(RAGGED, protocol, dev), protocol=protocol, method=method)
    torch.cuda.synchronize(dev)
    host = [{k: t.cpu().numpy() for k, t in r.items()} for r in res]
    _check_chain(host, RAGGED, protocol, method)
    if protocol == "scores":
        assert sum(int(h["user_selected"].sum()) for h in host) > 0 and host[2]["gtsummary"].sum() > 0


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_chain_on_poisoned_buffers_with_gaps(protocol):
    """Outputs and workspace pre-filled with 0xFF bytes, the videos' ranges 5 elements apart: the gaps stay 0xFF, the results are those of the
    packed layout, and a second run changes no byte."""
    from summarizer_amd.utils import annotate as M
    dev = _dev()
    chain = M.AnnotateChain(*_upload(RAGGED, protocol, dev), protocol=protocol, method="knapsack", _gap=5)
    chain.arena.fill_(255); chain.ws.fill_(255)
    chain.enqueue()
    first = chain.to_host()
    _check_chain(chain.views(first), RAGGED, protocol, "knapsack")
    for name, ranges in chain.layout.items():
        outside = np.ones(first[name].shape[0], bool)
        for lo, n in ranges:
            outside[lo:lo + n] = False
        assert outside.sum() == 5 * len(RAGGED) and np.all(first[name][outside].view(np.uint8) == 255), name
    first = {k: v.copy() for k, v in first.items()}
    chain.ws.fill_(255)
    chain.enqueue()
    second = chain.to_host()
    for name in first:
        assert_array_equal(first[name].view(np.uint8), second[name].view(np.uint8), err_msg=name)


def test_chain_replays_from_a_graph():
    """One capture of the four enqueued calls on fixed buffers (a single linear chain), one replay: the eager results, byte for byte."""
    from summarizer_amd.utils import annotate as M
    dev = _dev()
    vids = [VIDEOS[3], VIDEOS[1], VIDEOS[2]]
    chain = M.AnnotateChain(*_upload(vids, "scores", dev), protocol="scores", method="knapsack")
    chain.enqueue()
    eager = {k: v.copy() for k, v in chain.to_host().items()}
    _check_chain(chain.views(eager), vids, "scores", "knapsack")
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain.enqueue()
    chain.arena.fill_(255); chain.ws.fill_(255)
    g.replay()
    torch.cuda.synchronize(dev)
    replayed = chain.to_host()
    for name in eager:
        assert_array_equal(eager[name].view(np.uint8), replayed[name].view(np.uint8), err_msg=name)


def test_chain_refuses_what_python_can_see():
    from summarizer_amd._lib import SumkError
    from summarizer_amd.utils import annotate as M
    dev = _dev()
    annos, picks, nf, segs = _upload([VIDEOS[1]], "scores", dev)
    with pytest.raises(SumkError, match="GPU"):
        M.AnnotateChain([annos[0].cpu()], picks, nf, segs)
    with pytest.raises(SumkError, match="annotations"):
        M.AnnotateChain([annos[0][:, :16]], picks, nf, segs)
    with pytest.raises(SumkError, match="picks"):
        M.AnnotateChain(annos, [picks[0].long()], nf, segs)
    with pytest.raises(SumkError, match="segments"):
        M.AnnotateChain(annos, picks, nf, [(segs[0][0], segs[0][1][:2])])
    with pytest.raises(SumkError, match="annotators"):
        M.AnnotateChain([torch.ones(33, 17, device=dev)], picks, nf, segs)
    with pytest.raises(SumkError, match="score_range"):
        M.AnnotateChain(annos, picks, nf, segs, score_range=(3, 3))
    with pytest.raises(SumkError, match="summary_lens"):
        M.AnnotateChain(annos, picks, nf, segs, summary_lens=[17, 17])
    chain = M.AnnotateChain(annos, picks, nf, segs, summary_lens=[16])          # a host-known sum(n_frame_per_seg) that does not tile the frames:
    chain.arena.fill_(255)
    with pytest.raises(SumkError, match="tile"):                               # refused by sumk_annotate, nothing launched
        chain.enqueue()
    assert bool((chain.arena == 255).all())
    with pytest.raises(SumkError, match="tile"):
        M.annotate_batch(annos, picks, nf, segs, summary_lens=[18])
    with pytest.raises(SumkError, match="pending"):
        M.AnnotateChain(annos, picks, nf, [None])
    with pytest.raises(KeyError):
        M.AnnotateChain(annos, picks, nf, segs, protocol="grades")


# ------------------------------------------------------------------------------------------------ 4. build_records
def _irregular_picks(n, seed):
    rng = np.random.default_rng(seed)
    picks = np.cumsum(rng.integers(5, 25, size=n)).astype(np.int32)
    picks -= picks[0]
    return picks, int(picks[-1]) + int(rng.integers(3, 20))


@functools.lru_cache(maxsize=None)
def _raw_videos():
    """Three videos: two come without change points (small T, block-structured features: KTS finds the planted segments), one brings its own."""
    vids = {}
    for key, n, n_segs, seed in (("planted_a", 65, 4, 301), ("planted_b", 90, 6, 302), ("own_segments", 40, 3, 303)):
        X, _ = kts_ref.planted_features(n, 128, n_segs, 0.05, seed)
        picks, n_frames = _irregular_picks(n, seed)
        vids[key] = {"features": X, "picks": picks, "n_frames": n_frames, "video_name": np.array(key + ".mp4")}
    nf = vids["own_segments"]["n_frames"]
    lengths = [50] * (nf // 50 - 1) + [nf - 50 * (nf // 50 - 1)]
    vids["own_segments"]["change_points"], vids["own_segments"]["n_frame_per_seg"] = A.segments_of_lengths(lengths)
    return vids


def _with_annotations(protocol):
    make = A.block_grades if protocol == "scores" else A.block_selections
    return {k: dict(v, annotations=make(4, v["n_frames"], 400 + i)) for i, (k, v) in enumerate(_raw_videos().items())}


@functools.lru_cache(maxsize=None)
def _host_segments(key):
    from summarizer_amd.utils.kts import cps_to_segments
    v = _raw_videos()[key]
    if "change_points" in v:
        return v["change_points"], v["n_frame_per_seg"]
    X = v["features"].astype(np.float64)
    cps, _ = kts_ref.cpd_auto(X @ X.T, 89)                       # max_ncp of the call: the longest video without segments, 90 steps, minus one
    return cps_to_segments(cps, v["picks"], v["n_frames"])


def _trainer(ds, keys, **over):
    from summarizer_amd.models.vasnet import VASNetTrainer
    from summarizer_amd.utils.hps import make_hps
    hps = make_hps(ds, [{"train_keys": [], "test_keys": keys}], epochs=1, extra_params={"input_size": "128"}, **over)
    torch.manual_seed(77)
    return VASNetTrainer(hps, hps.splits_files[0]).reset()


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_build_records_with_kts(protocol):
    from summarizer_amd.utils import annotate as M
    from summarizer_amd.utils.datasets import DictDataset
    vids = _with_annotations(protocol)
    ds = M.build_records(vids, protocol=protocol)
    assert isinstance(ds, DictDataset) and list(ds.keys()) == list(vids.keys())
    for key, v in vids.items():
        cp, nfps = _host_segments(key)
        assert len(cp) > 1
        want = A.record(v["annotations"], v["picks"], v["n_frames"], cp, nfps, protocol)
        rec = ds[key]
        assert sorted(rec.keys()) == sorted(["features", "picks", "n_frames", "n_steps", "change_points", "n_frame_per_seg", "user_scores", "user_summary",
                                             "gtscore", "gtsummary", "video_name"])
        assert_array_equal(rec["change_points"][...], cp); assert_array_equal(rec["n_frame_per_seg"][...], nfps)
        assert rec["change_points"][...].dtype == np.int32 and rec["n_frame_per_seg"][...].dtype == np.int32
        for f in ("user_scores", "user_summary", "gtscore", "gtsummary"):
            assert_array_equal(rec[f][...], want[f], err_msg=f"{key} {f}")
            assert rec[f][...].dtype == F32
        assert_array_equal(rec["features"][...], v["features"]); assert_array_equal(rec["picks"][...], v["picks"])
        assert int(rec["n_frames"][()]) == v["n_frames"] and int(rec["n_steps"][()]) == v["features"].shape[0]
        assert str(rec["video_name"][()]) == key + ".mp4"
        assert rec["user_summary"][...].shape == (4, v["n_frames"]) and rec["gtsummary"][...].shape == rec["gtscore"][...].shape == (len(v["picks"]),)
    metrics = _trainer(ds, list(vids.keys())).test(0)             # a trainer opens the records unchanged
    assert np.isfinite(metrics[0]) and np.isfinite(metrics[1][0]) and np.isfinite(metrics[1][1])


def test_build_records_names_the_video_and_the_row_of_a_device_status():
    """Only the device sees a segment mean past 1e12 (grades of 1e20 on a [0, 1] scale): SelectStatusError with the video and the row."""
    from summarizer_amd._lib import SumkError
    from summarizer_amd.utils import annotate as M
    vids = _with_annotations("scores")
    vids["own_segments"]["annotations"] = vids["own_segments"]["annotations"].copy()
    vids["own_segments"]["annotations"][2] = 1e20
    assert issubclass(M.SelectStatusError, SumkError)
    with pytest.raises(M.SelectStatusError, match=r"video own_segments, row 2 \(annotator 2\).*status 1"):
        M.build_records(vids, score_range=(0, 1))


def test_command_line(tmp_path, capsys):
    from summarizer_amd.utils import annotate as M
    from summarizer_amd.utils.datasets import DictDataset, open_dataset
    vids = _with_annotations("summaries")
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    DictDataset(vids).save_npz(src)
    assert M.main([src, dst, "--protocol", "summaries", "--method", "rank"]) == 0
    assert "3 records" in capsys.readouterr().out
    want, got = M.build_records(vids, protocol="summaries", method="rank"), open_dataset(dst)
    assert sorted(got.keys()) == sorted(want.keys())
    for key in want:
        assert sorted(got[key].keys()) == sorted(want[key].keys())
        for f in want[key]:
            assert_array_equal(got[key][f][...], want[key][f][...], err_msg=f"{key} {f}")
