"""GPU: rank correlation for long videos (csrc/evalcorr_long.hip: sumk_eval_device_spearman_long, sumk_eval_device_kendall_long),
`evaluate_batch_device(tail="long")` and `hps.eval_tail = "long"`.

References.  Kendall: the host tail `sumk_eval_videos_kendall` -- tau, its mean and the counts {cmd, xtie, ytie, ntie} with
`assert_array_equal` -- and, where the input fits, the one-workgroup kernel `sumk_eval_device_kendall`, again bit for bit.  Spearman:
`sumk_eval_device_spearman` to atol 1e-12 where both accept the input (the gate tests/test_gpu_evaltail.py holds between the block forms);
everywhere the exact oracle of tests/corr_long_common.py under that file's rule: the device's distance from the oracle is at most
max(4 x the host tail's own distance on the same videos, 1e-12).  The worst ratio (device distance / that bound) of every Spearman case is
printed and kept in REPORT (written to $SUMK_REPORT_DIR/corr_long.json when set).  Measured on MI355X (the same with
SUMK_TEST_POISON=1): in every case the device's distance from the oracle equals the host tail's -- 1.7e-18 (sizes), 6.9e-18 (frame
edges), 2.2e-19 (300 000 frames x 32 annotators), 2.6e-18 (batches), 3.5e-18 (trainer) -- a ratio to the bound below 1e-5.
All workspace and output buffers start as 0xFF bytes."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import corr_long_common as K

pytestmark = pytest.mark.gpu

TILE = K.TILE
OLD_MAX_INT, OLD_MAX_FRAMES = 4096, 16384      # ED_MAX_INT / KD_MAX_FRAMES: what the one-workgroup kernels take
REPORT = {}


def _dev():
    return torch.device("cuda:0")


def _poisoned(numel, dtype, dev):
    t = torch.empty(max(int(numel), 1), dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(255)
    return t


def _all_ff(t):
    return bool((t.view(torch.uint8) == 255).all().item())


def _report(case, got, host):
    bound = max(4 * host, 1e-12)
    REPORT[case] = dict(device_minus_oracle=got, host_minus_oracle=host, ratio=got / bound)
    print(f"CORR_LONG {case}: max |device - oracle| = {got:.3e}, max |host tail - oracle| = {host:.3e}, ratio to the bound = {got / bound:.3f}")
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "corr_long.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _spearman_gate(case, corr_dev, corr_host, corr_ref):
    """tests/test_gpu_evaltail.py _check_against_oracle: 4 x the host tail's own distance from the oracle on these videos, floor 1e-12."""
    nan = np.isnan(corr_ref)
    assert np.array_equal(np.isnan(corr_dev), nan), (case, corr_dev, corr_ref)
    assert np.array_equal(np.isnan(corr_host), nan), (case, corr_host, corr_ref)
    if nan.all():
        return
    host = float(np.abs(corr_host[~nan] - corr_ref[~nan]).max())
    got = float(np.abs(corr_dev[~nan] - corr_ref[~nan]).max())
    _report(case, got, host)
    assert got <= max(4 * host, 1e-12), (case, got, host)


def _oracle(raws, vids, scores=None):
    scores = [r["scores"] for r in raws] if scores is None else scores
    return np.array([K.exact_spearman(s, r["n_frames"], r["picks"], v["user_ranks"]) for r, v, s in zip(raws, vids, scores)])


def _corr_call(vids, scores, metric, entry="long", ws_short=0, override=None, dev_override=None, null=()):
    """One of the four C entries on buffers of the test's own, all of them 0xFF first.  vids: prepare_video dicts; scores: one float32
    array per video.  override: {video: {field: value}} on the HOST AND DEVICE copy of the descriptors; dev_override: on the device copy
    alone (what the entry point cannot see); null: arguments passed as null pointers."""
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    lib, dev, n = _lib.load(), _dev(), len(vids)
    kendall = metric == "kendalltau"
    packed = torch.from_numpy(np.concatenate([np.asarray(s, np.float32) for s in scores])).to(dev)
    descr, kd = (_lib.EvalDevVideo * n)(), (_lib.EvalDevKendall * n)()
    keep, row0, frame0, users = [], 0, 0, 0
    for i, (v, s) in enumerate(zip(vids, scores)):
        m = eval_native._device_meta(v, dev, kendall=kendall); keep.append(m)
        e = descr[i]
        e.picks, e.n_picks, e.n_frames, e.n_steps = m["picks"].data_ptr(), v["picks"].shape[0], v["n_frames"], len(s)
        e.row0, e.frame0 = row0, frame0
        e.user_ranks, e.user_mean, e.user_ssq, e.n_users = m["ranks"].data_ptr(), m["mean"].data_ptr(), m["ssq"].data_ptr(), v["user_ranks"].shape[0]
        if kendall:
            kd[i].y_dense, kd[i].ytie, kd[i].counts0 = m["ydense"].data_ptr(), m["ytie"].data_ptr(), users
        row0 += len(s); frame0 += v["n_frames"]; users += v["user_ranks"].shape[0]
    on_dev = (_lib.EvalDevVideo * n).from_buffer_copy(bytes(descr))          # (the size query and the workspace go by the videos as they are)
    ws_bytes = (lib.sumk_eval_device_kendall_long_workspace_bytes if kendall else lib.sumk_eval_device_spearman_long_workspace_bytes)(C.cast(descr, C.c_void_p), n)
    assert ws_bytes > 0
    for i, fields in (override or {}).items():
        for k, val in fields.items():
            setattr(descr[i], k, val); setattr(on_dev[i], k, val)
    for i, fields in (dev_override or {}).items():
        for k, val in fields.items():
            setattr(on_dev[i], k, val)
    descr_dev = torch.frombuffer(bytearray(bytes(on_dev)), dtype=torch.uint8).to(dev)
    kd_dev = torch.frombuffer(bytearray(bytes(kd)), dtype=torch.uint8).to(dev)
    corr, counts = _poisoned(n, torch.float64, dev), _poisoned(4 * users, torch.int64, dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if entry == "block":
        if kendall:
            ws = _poisoned(lib.sumk_eval_device_kendall_scratch_bytes(n, frame0), torch.uint8, dev)
            rc = lib.sumk_eval_device_kendall(packed.data_ptr(), descr_dev.data_ptr(), kd_dev.data_ptr(), n, ws.data_ptr(), corr.data_ptr(), counts.data_ptr(), st)
        else:
            ws = _poisoned(lib.sumk_eval_device_spearman_scratch_bytes(n), torch.uint8, dev)
            rc = lib.sumk_eval_device_spearman(packed.data_ptr(), descr_dev.data_ptr(), n, ws.data_ptr(), corr.data_ptr(), st)
    else:
        ws = _poisoned(ws_bytes, torch.uint8, dev)
        ptr = dict(scores=packed.data_ptr(), descr_dev=descr_dev.data_ptr(), descr=C.cast(descr, C.c_void_p), kd=kd_dev.data_ptr(), ws=ws.data_ptr(),
                   corr=corr.data_ptr(), counts=counts.data_ptr())
        for k in null:
            ptr[k] = None
        if kendall:
            rc = lib.sumk_eval_device_kendall_long(ptr["scores"], ptr["descr_dev"], ptr["descr"], ptr["kd"], n, ptr["ws"], ws_bytes - ws_short, ptr["corr"],
                                                   ptr["counts"], st)
        else:
            rc = lib.sumk_eval_device_spearman_long(ptr["scores"], ptr["descr_dev"], ptr["descr"], n, ptr["ws"], ws_bytes - ws_short, ptr["corr"], st)
    torch.cuda.synchronize(dev)
    per = [v["user_ranks"].shape[0] for v in vids]
    flat = counts.cpu().numpy()[:4 * users].reshape(-1, 4)
    return dict(rc=rc, corr=corr.cpu().numpy(), counts=np.split(flat, np.cumsum(per)[:-1]), error=lib.sumk_last_error().decode(errors="replace"),
                untouched=_all_ff(corr) and _all_ff(counts) and _all_ff(ws))


def _host(vids, scores, metric):
    from summarizer_amd.utils import eval_native
    co = []
    corr = eval_native.evaluate_batch(vids, scores, metric=metric, counts_out=co if metric == "kendalltau" else None, n_threads=4)[0]
    return corr, co


def _n_int(v):
    return v["picks"].shape[0] - 1 + (1 if v["picks"][-1] != v["n_frames"] else 0)


# ------------------------------------------------------------------------------------------------ 1. sizes
@pytest.fixture(scope="module")
def size_batch():
    """One video per pick count of K.PICK_SIZES, 15 frames per pick, videos of 1 pick and of 5 TILE + 3 picks side by side in one call; the
    last pick alternately below and equal to n_frames."""
    raws = [K.make_video(p, 100 + i, n_users=3, tail=9 if i in (0, 2, 4, 6) else 0) for i, p in enumerate(K.PICK_SIZES)]
    vids = [K.prepare(r) for r in raws]
    assert any(_n_int(v) == v["picks"].shape[0] for v in vids) and any(_n_int(v) == v["picks"].shape[0] - 1 for v in vids)
    assert all(r["n_steps"] < _n_int(v) for r, v in zip(raws, vids) if _n_int(v) > 3)
    return raws, vids, [r["scores"] for r in raws]


def test_spearman_long_sizes(size_batch):
    raws, vids, scores = size_batch
    got = _corr_call(vids, scores, "spearmanr")
    assert got["rc"] == 0, got["error"]
    fits = [i for i, v in enumerate(vids) if _n_int(v) <= OLD_MAX_INT]
    assert len(fits) >= 7 and len(fits) < len(vids)
    block = _corr_call([vids[i] for i in fits], [scores[i] for i in fits], "spearmanr", entry="block")
    assert block["rc"] == 0
    np.testing.assert_allclose(got["corr"][fits], block["corr"], rtol=0, atol=1e-12)
    host, _ = _host(vids, scores, "spearmanr")
    _spearman_gate("sizes", got["corr"], host, _oracle(raws, vids))
    # a video's result does not depend on its neighbours
    alone = _corr_call(vids[-1:], scores[-1:], "spearmanr")
    np.testing.assert_array_equal(alone["corr"], got["corr"][-1:])


def test_kendall_long_sizes(size_batch):
    raws, vids, scores = size_batch
    got = _corr_call(vids, scores, "kendalltau")
    assert got["rc"] == 0, got["error"]
    host, counts = _host(vids, scores, "kendalltau")
    np.testing.assert_array_equal(got["corr"], host)
    for i, (a, b) in enumerate(zip(got["counts"], counts)):
        np.testing.assert_array_equal(a, b, err_msg=f"{K.PICK_SIZES[i]} picks")
    assert np.isfinite(host).sum() >= 8
    fits = [i for i, v in enumerate(vids) if _n_int(v) <= OLD_MAX_INT and v["n_frames"] <= OLD_MAX_FRAMES]
    assert fits
    block = _corr_call([vids[i] for i in fits], [scores[i] for i in fits], "kendalltau", entry="block")
    np.testing.assert_array_equal(got["corr"][fits], block["corr"])
    for k, i in enumerate(fits):
        np.testing.assert_array_equal(got["counts"][i], block["counts"][k])


@pytest.fixture(scope="module")
def frame_batch():
    frames = (OLD_MAX_FRAMES - 1, OLD_MAX_FRAMES, OLD_MAX_FRAMES + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 3)
    raws = [K.video_of_frames(f, 200 + i, n_users=2 + i % 3) for i, f in enumerate(frames)]
    assert [r["n_frames"] for r in raws] == list(frames)
    return raws, [K.prepare(r) for r in raws], [r["scores"] for r in raws]


def test_kendall_long_frame_tile_edges(frame_batch):
    """The frame keys' sort on the edges of its LDS tile and of the one-workgroup kernel's 16 384 frames."""
    raws, vids, scores = frame_batch
    got = _corr_call(vids, scores, "kendalltau")
    assert got["rc"] == 0, got["error"]
    host, counts = _host(vids, scores, "kendalltau")
    np.testing.assert_array_equal(got["corr"], host)
    for a, b, r in zip(got["counts"], counts, raws):
        np.testing.assert_array_equal(a, b, err_msg=f"{r['n_frames']} frames")
    assert np.isfinite(host).all()
    fits = [i for i, v in enumerate(vids) if v["n_frames"] <= OLD_MAX_FRAMES]
    block = _corr_call([vids[i] for i in fits], [scores[i] for i in fits], "kendalltau", entry="block")
    np.testing.assert_array_equal(got["corr"][fits], block["corr"])
    for k, i in enumerate(fits):
        np.testing.assert_array_equal(got["counts"][i], block["counts"][k])


def test_spearman_long_frame_edges(frame_batch):
    raws, vids, scores = frame_batch
    got = _corr_call(vids, scores, "spearmanr")
    assert got["rc"] == 0, got["error"]
    block = _corr_call(vids, scores, "spearmanr", entry="block")
    np.testing.assert_allclose(got["corr"], block["corr"], rtol=0, atol=1e-12)
    host, _ = _host(vids, scores, "spearmanr")
    _spearman_gate("frame_edges", got["corr"], host, _oracle(raws, vids))


@pytest.fixture(scope="module")
def big_video():
    r = K.video_of_frames(300000, 300, n_users=32)
    return [r], [K.prepare(r)], [r["scores"]]


def test_spearman_long_300k_frames_32_annotators(big_video):
    raws, vids, scores = big_video
    got = _corr_call(vids, scores, "spearmanr")
    assert got["rc"] == 0, got["error"]
    host, _ = _host(vids, scores, "spearmanr")
    _spearman_gate("300k_frames_32_annotators", got["corr"], host, _oracle(raws, vids))


def test_kendall_long_300k_frames_32_annotators(big_video):
    raws, vids, scores = big_video
    got = _corr_call(vids, scores, "kendalltau")
    assert got["rc"] == 0, got["error"]
    host, counts = _host(vids, scores, "kendalltau")
    np.testing.assert_array_equal(got["corr"], host)
    np.testing.assert_array_equal(got["counts"][0], counts[0])
    assert np.isfinite(host).all() and (counts[0][:, 3] > 0).any()


# ------------------------------------------------------------------------------------------------ 2. NaN
def test_constant_sides_and_a_nan_annotator():
    raws = [K.make_video(p, 400 + i, n_users=3) for i, p in enumerate((50, TILE + 5, 60))]
    # video 0: every score 0 -- with the uncovered frames one tie group: a constant machine side
    raws[0]["scores"][:] = 0.0
    # video 1: annotator 1 gives every frame the same grade: that annotator's value, and so the video's mean, is NaN
    raws[1]["user_scores"][1, :] = 3.0
    vids = [K.prepare(r) for r in raws]
    scores = [r["scores"] for r in raws]
    for metric in ("kendalltau", "spearmanr"):
        got = _corr_call(vids, scores, metric)
        assert got["rc"] == 0, got["error"]
        assert np.isnan(got["corr"][0]) and np.isnan(got["corr"][1]) and np.isfinite(got["corr"][2]), (metric, got["corr"])
        if metric == "spearmanr":                                                     # NaN where sumk_eval_device_spearman gives NaN
            block = _corr_call(vids, scores, metric, entry="block")
            assert np.array_equal(np.isnan(block["corr"]), np.isnan(got["corr"])), block["corr"]
            np.testing.assert_allclose(got["corr"][2], block["corr"][2], rtol=0, atol=1e-12)
        if metric == "kendalltau":
            host, counts = _host(vids, scores, metric)
            np.testing.assert_array_equal(got["corr"], host)
            for a, b in zip(got["counts"], counts):
                np.testing.assert_array_equal(a, b)
            n = vids[0]["n_frames"]
            assert (got["counts"][0][:, 1] == n * (n - 1) // 2).all()                 # xtie == tot
            n = vids[1]["n_frames"]
            assert got["counts"][1][1, 2] == n * (n - 1) // 2 and (got["counts"][1][[0, 2], 2] < n * (n - 1) // 2).all()


# ------------------------------------------------------------------------------------------------ 3. refusals
@pytest.fixture(scope="module")
def small_batch():
    raws = [K.make_video(p, 500 + i, n_users=2 + i) for i, p in enumerate((30, 4100, 77))]
    return raws, [K.prepare(r) for r in raws], [r["scores"] for r in raws]


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_refusals_launch_nothing(metric, small_batch):
    raws, vids, scores = small_batch
    cases = [(dict(override={1: dict(n_picks=(1 << 20) + 1)}), "picks"), (dict(override={1: dict(n_picks=0)}), "0 picks"),
             (dict(override={2: dict(n_frames=(1 << 24) + 1)}), "frames"), (dict(override={0: dict(n_frames=0)}), "0 frames"),
             (dict(override={0: dict(n_users=33)}), "33 annotators"), (dict(override={0: dict(picks=None)}), "no picks"),
             (dict(ws_short=1), "workspace")]
    cases += [(dict(null=(k,)), "null pointer") for k in ("scores", "descr_dev", "descr", "ws", "corr") + (("kd",) if metric == "kendalltau" else ())]
    for kw, word in cases:
        r = _corr_call(vids, scores, metric, **kw)
        assert r["rc"] == -1 and word in r["error"], (kw, r["error"])
        assert r["untouched"], kw


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_a_bad_device_descriptor_is_nan_for_that_video_only(metric, small_batch):
    raws, vids, scores = small_batch
    others = _corr_call([vids[0], vids[2]], [scores[0], scores[2]], metric)
    assert others["rc"] == 0 and np.isfinite(others["corr"]).all()
    for fields in (dict(n_picks=(1 << 20) + 1), dict(n_frames=(1 << 24) + 1), dict(n_picks=0), dict(n_frames=vids[1]["n_frames"] + 1),
                   dict(n_picks=vids[1]["picks"].shape[0] + 1)):
        r = _corr_call(vids, scores, metric, dev_override={1: fields})
        assert r["rc"] == 0, r["error"]
        assert np.isnan(r["corr"][1]), fields
        np.testing.assert_array_equal(r["corr"][[0, 2]], others["corr"])
        if metric == "kendalltau":
            assert (r["counts"][1] == -1).all(), fields
            np.testing.assert_array_equal(r["counts"][0], others["counts"][0]); np.testing.assert_array_equal(r["counts"][2], others["counts"][1])


# ------------------------------------------------------------------------------------------------ 4. evaluate_batch_device(tail="long")
@pytest.fixture(scope="module")
def fold_batch():
    raws = [K.make_video(p, 600 + i, n_users=4 + i) for i, p in enumerate((5000, 300, 4097))]
    return raws, [K.prepare(r) for r in raws], [r["scores"] for r in raws]


def _check_batch(case, got, want, metric, raws, vids, scores, counts_got=None, counts_want=None):
    np.testing.assert_array_equal(got[1], want[1]); np.testing.assert_array_equal(got[2], want[2])
    for a, b in zip(got[3], want[3]):
        np.testing.assert_array_equal(a, b)
    if metric == "kendalltau":
        np.testing.assert_array_equal(got[0], want[0])
        assert len(counts_got) == len(counts_want) == len(vids)
        for a, b in zip(counts_got, counts_want):
            np.testing.assert_array_equal(a, b)
    else:
        _spearman_gate(case, got[0], want[0], _oracle(raws, vids, scores))


@pytest.mark.parametrize("select", ["host", "device"])
@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_evaluate_batch_device_long_equals_the_host_tail(metric, select, fold_batch):
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    raws, vids, scores = fold_batch
    dev, lens = _dev(), [len(s) for s in scores]
    packed = torch.from_numpy(np.concatenate(scores)).to(dev)
    with pytest.raises(_lib.SumkError):                                                       # the block tail refuses the batch
        eval_native.evaluate_batch_device(vids, packed, lens, metric=metric, select=select)
    cw, cg = [], []
    want = eval_native.evaluate_batch(vids, scores, 0.15, "knapsack", want_summaries=True, metric=metric, counts_out=cw if metric == "kendalltau" else None)
    got = eval_native.evaluate_batch_device(vids, packed, lens, 0.15, "knapsack", want_summaries=True, metric=metric,
                                            counts_out=cg if metric == "kendalltau" else None, select=select, tail="long")
    _check_batch(f"batch_{select}", got, want, metric, raws, vids, scores, cg, cw)
    # the cached entry with its buffers poisoned, other scores, the rank method
    ent = eval_native._DEV_BATCH_CACHE[(tuple(id(v) for v in vids), tuple(lens), str(dev), "long")]
    for t in list(ent["buffers"].values()) + [w["ws"] for w in ent["corr_ws"].values()] + [s[k] for s in ent["select"].values() for k in ("ws", "res", "summary", "selected")]:
        if torch.is_tensor(t) and t.is_cuda:
            t.view(torch.uint8).fill_(255)
    rng = np.random.default_rng(61)
    scores2 = [(rng.integers(0, 33, size=len(s)) / 32.0).astype(np.float32) for s in scores]
    want2 = eval_native.evaluate_batch(vids, scores2, 0.15, "rank", want_summaries=True, metric=metric, counts_out=cw if metric == "kendalltau" else None)
    got2 = eval_native.evaluate_batch_device(vids, torch.from_numpy(np.concatenate(scores2)).to(dev), lens, 0.15, "rank", want_summaries=True, metric=metric,
                                             counts_out=cg if metric == "kendalltau" else None, select=select, tail="long")
    _check_batch(f"batch_{select}_again", got2, want2, metric, raws, vids, scores2, cg, cw)


@pytest.mark.parametrize("select", ["host", "device"])
@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_long_tail_equals_block_tail_inside_the_block_limits(metric, select):
    import recipes as R
    from summarizer_amd.utils import eval as E
    from summarizer_amd.utils import eval_native
    dev = _dev()
    rng = np.random.default_rng(62)
    vids, scores = [], []
    for i, (T, U) in enumerate([(300, 15), (1, 3), (97, 20), (650, 18), (320, 32)]):
        v = R.synthetic_video(T, 8900 + i, n_users=U)
        vids.append(eval_native.prepare_video(v["n_frames"], v["picks"], v["change_points"], v["n_frame_per_seg"], v["user_summary"], E.rank_users(v["user_scores"])))
        scores.append((rng.integers(0, 17, size=T) / 16.0).astype(np.float32))
    lens = [len(s) for s in scores]
    packed = torch.from_numpy(np.concatenate(scores)).to(dev)
    cb, cl = [], []
    kw = dict(want_summaries=True, metric=metric, select=select)
    block = eval_native.evaluate_batch_device(vids, packed, lens, 0.15, "knapsack", counts_out=cb if metric == "kendalltau" else None, **kw)
    long_ = eval_native.evaluate_batch_device(vids, packed, lens, 0.15, "knapsack", counts_out=cl if metric == "kendalltau" else None, tail="long", **kw)
    np.testing.assert_array_equal(long_[1], block[1]); np.testing.assert_array_equal(long_[2], block[2])
    for a, b in zip(long_[3], block[3]):
        np.testing.assert_array_equal(a, b)
    if metric == "kendalltau":
        np.testing.assert_array_equal(long_[0], block[0])
        for a, b in zip(cl, cb):
            np.testing.assert_array_equal(a, b)
    else:
        np.testing.assert_allclose(long_[0], block[0], rtol=0, atol=1e-12)


def test_a_tiny_workspace_budget_raises_before_anything_is_enqueued(monkeypatch):
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    raws = [K.make_video(p, 700 + i) for i, p in enumerate((200, 90))]
    vids, scores = [K.prepare(r) for r in raws], [r["scores"] for r in raws]
    lens = [len(s) for s in scores]
    packed = torch.from_numpy(np.concatenate(scores)).to(_dev())
    lib = _lib.load()
    launched = []
    for name in ("sumk_eval_device_segments_long", "sumk_eval_device_spearman_long", "sumk_eval_device_kendall_long", "sumk_eval_device_select_long"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0, raising=True)
    for metric in ("spearmanr", "kendalltau"):
        need = eval_native.corr_long_workspace_bytes([(v["picks"].shape[0], v["n_frames"], v["user_ranks"].shape[0]) for v in vids], metric)
        with pytest.raises(_lib.SumkError, match=str(need)):
            eval_native.evaluate_batch_device(vids, packed, lens, metric=metric, tail="long", max_workspace_bytes=1000)
        with pytest.raises(_lib.SumkError, match=f"{need} bytes"):
            eval_native.evaluate_batch_device(vids, packed, lens, metric=metric, tail="long", select="device", max_workspace_bytes=need - 1)
    assert launched == []


# ------------------------------------------------------------------------------------------------ 5. Trainer.test
def _fold_dataset():
    from summarizer_amd.utils.datasets import DictDataset
    rng = np.random.default_rng(63)
    videos = {}
    for i, T in enumerate((5000, 300, 4097)):
        n_frames = 15 * T - 4
        picks = (15 * np.arange(T)).astype(np.int32)
        S = 30
        cuts = np.sort(rng.choice(np.arange(15, n_frames - 15), size=S - 1, replace=False))
        starts, ends = np.concatenate([[0], cuts]), np.concatenate([cuts - 1, [n_frames - 1]])
        gt = rng.random(T).astype(np.float32)
        feats = 0.5 * np.abs(rng.standard_normal((T, 64))).astype(np.float32)
        feats[:, :8] += gt[:, None]
        users = np.repeat(np.round(np.clip(gt[None, :] + 0.3 * rng.standard_normal((4, T)), 0, 1) * 4) / 4, 15, axis=1)[:, :n_frames].astype(np.float32)
        videos[f"video_{i + 1}"] = dict(features=feats, gtscore=gt, user_scores=users, user_summary=(rng.random((4, n_frames)) < 0.15).astype(np.float32),
                                       change_points=np.stack([starts, ends], axis=1).astype(np.int32), n_frame_per_seg=(ends - starts + 1).astype(np.int32),
                                       n_frames=np.int64(n_frames), n_steps=np.int64(T), picks=picks)
    return DictDataset(videos)


def _trainer(ds, keys, **over):
    from summarizer_amd.models.logistic import LogisticRegressionTrainer
    from summarizer_amd.utils.hps import make_hps
    hps = make_hps(ds, [{"train_keys": [], "test_keys": keys}], epochs=1, extra_params={"input_size": "64"}, **over)
    torch.manual_seed(78)
    return LogisticRegressionTrainer(hps, hps.splits_files[0]).reset()


@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_trainer_eval_tail_long(metric, monkeypatch):
    from summarizer_amd.utils import eval_native
    ds = _fold_dataset()
    keys = ["video_1", "video_2", "video_3"]
    seen = {}
    real_host, real_dev = eval_native.evaluate_batch, eval_native.evaluate_batch_device

    def spy_host(*a, **k):
        seen["host"] = real_host(*a, **k)
        return seen["host"]

    def spy_dev(*a, **k):
        seen["dev"] = (k, real_dev(*a, **k))
        return seen["dev"][1]
    monkeypatch.setattr(eval_native, "evaluate_batch", spy_host)
    monkeypatch.setattr(eval_native, "evaluate_batch_device", spy_dev)
    plain = _trainer(ds, keys, correlation_metric=metric)
    default = plain.test(0)
    assert "host" in seen and "dev" not in seen                                    # 5000 picks: the block tail hands the fold to the host
    t = _trainer(ds, keys, correlation_metric=metric, eval_tail="long")
    returned = []
    real_tod = t._test_on_device
    monkeypatch.setattr(t, "_test_on_device", lambda *a, **k: returned.append(real_tod(*a, **k)) or returned[-1])
    long_ = t.test(0)
    assert len(returned) == 1 and returned[0] is not None and seen["dev"][0]["tail"] == "long"
    assert long_[1] == default[1]                                                  # F-scores: bit-equal
    host_corr, dev_corr = seen["host"][0], seen["dev"][1][0]
    if metric == "kendalltau":
        np.testing.assert_array_equal(dev_corr, host_corr)
        assert long_[0] == default[0]
    else:
        sc = plain._score_keys(keys)
        metas = [plain._native_meta(k) for k in keys]
        ref = np.array([K.exact_spearman(sc[k], m["n_frames"], m["picks"], m["user_ranks"]) for k, m in zip(keys, metas)])
        _spearman_gate("trainer", dev_corr, host_corr, ref)
        assert abs(long_[0] - default[0]) <= 1e-12
    # scored in groups of at most max_frames_per_launch steps: the same numbers
    f_avg = seen["dev"][1][1]
    grouped = real_tod(keys, max_frames_per_launch=5000)
    np.testing.assert_array_equal(grouped[0], dev_corr); np.testing.assert_array_equal(grouped[1], f_avg)


def test_trainer_default_tail_is_unchanged(monkeypatch):
    """Without hps.eval_tail the block tail runs as before: one packed scoring launch of all the fold's steps, one evaluate_batch_device
    call with today's arguments (no `tail`)."""
    from summarizer_amd.utils import eval_native
    from summarizer_amd.utils.datasets import synthetic_dataset
    ds = synthetic_dataset(4, seed=44, D=64, t_range=(30, 90), n_users=3)
    keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
    t = _trainer(ds, keys)
    calls, packs = [], []
    real = eval_native.evaluate_batch_device
    monkeypatch.setattr(eval_native, "evaluate_batch_device", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    real_score = t.model.score_packed
    monkeypatch.setattr(t.model, "score_packed", lambda x, lens: (packs.append((x.shape[0], list(lens))), real_score(x, lens))[1])
    res = t.test(0)
    total = sum(int(ds[k]["n_steps"][()]) for k in keys)
    assert calls == [dict(metric="spearmanr", select="host")] and len(packs) == 1 and packs[0][0] == total and len(packs[0][1]) == 4
    assert np.isfinite(res[0])
    with pytest.raises(KeyError, match="Unknown tail"):
        _trainer(ds, keys, eval_tail="tall").test(0)


# ------------------------------------------------------------------------------------------------ 6. graph capture
@pytest.mark.parametrize("metric", ["spearmanr", "kendalltau"])
def test_long_chain_replays_from_a_graph(metric):
    """segments_long + the long correlation + select_long on fixed buffers: one linear graph, replayed twice with new scores; each replay
    equals the eager call on the same scores bit for bit (the pattern of test_long_segments_and_select_replay_from_a_graph)."""
    from summarizer_amd import _lib
    from summarizer_amd.utils import eval_native
    lib, dev = _lib.load(), _dev()
    kendall = metric == "kendalltau"
    raws = [K.make_video(p, 800 + i, n_users=2 + i) for i, p in enumerate((120, TILE + 40, 45))]
    vids = [K.prepare(r) for r in raws]
    lens, n = [r["n_steps"] for r in raws], 3
    vd, sd, kd = (_lib.EvalDevVideo * n)(), (_lib.EvalDevSelect * n)(), (_lib.EvalDevKendall * n)()
    metas = [eval_native._device_meta(v, dev, select=True) for v in vids]
    kmetas = [eval_native._device_meta(v, dev, kendall=True) for v in vids]
    segs, frames = sum(v["cps"].shape[0] for v in vids), sum(v["n_frames"] for v in vids)
    users = sum(v["user_ranks"].shape[0] for v in vids)
    scores = torch.zeros(sum(lens), dtype=torch.float32, device=dev)
    total = sum(int(v["nfps"].sum()) for v in vids)
    row0 = frame0 = seg0 = at = u0 = 0
    seg = _poisoned(segs, torch.float32, dev)
    for i, (v, m, T) in enumerate(zip(vids, metas, lens)):
        e, q = vd[i], sd[i]
        e.picks, e.n_picks, e.n_frames, e.n_steps, e.row0, e.frame0 = m["picks"].data_ptr(), v["picks"].shape[0], v["n_frames"], T, row0, frame0
        e.cps, e.n_segs, e.seg0 = m["cps"].data_ptr(), v["cps"].shape[0], seg0
        e.user_ranks, e.user_mean, e.user_ssq, e.n_users = m["ranks"].data_ptr(), m["mean"].data_ptr(), m["ssq"].data_ptr(), v["user_ranks"].shape[0]
        q.seg_means, q.nfps, q.n_segs, q.n_frames = seg.data_ptr() + 4 * seg0, m["nfps"].data_ptr(), v["cps"].shape[0], v["n_frames"]
        q.capacity, q.summary_len, q.summary0, q.sel0 = eval_native.select_capacity(v["n_frames"], 0.15), int(v["nfps"].sum()), at, seg0
        q.user_mask, q.n_users, q.method = m["mask"].data_ptr(), m["mask"].shape[0], 0
        kd[i].y_dense, kd[i].ytie, kd[i].counts0 = kmetas[i]["ydense"].data_ptr(), kmetas[i]["ytie"].data_ptr(), u0
        row0 += T; frame0 += v["n_frames"]; seg0 += v["cps"].shape[0]; at += q.summary_len; u0 += v["user_ranks"].shape[0]
    vd_dev = torch.frombuffer(bytearray(bytes(vd)), dtype=torch.uint8).to(dev)
    sd_dev = torch.frombuffer(bytearray(bytes(sd)), dtype=torch.uint8).to(dev)
    kd_dev = torch.frombuffer(bytearray(bytes(kd)), dtype=torch.uint8).to(dev)
    size_of = lib.sumk_eval_device_kendall_long_workspace_bytes if kendall else lib.sumk_eval_device_spearman_long_workspace_bytes
    out = dict(scratch=_poisoned(frames, torch.float32, dev), seg=seg, summary=_poisoned(total, torch.float32, dev), selected=_poisoned(segs, torch.uint8, dev),
               f=_poisoned(2 * n, torch.float64, dev), status=_poisoned(n, torch.int32, dev), corr=_poisoned(n, torch.float64, dev),
               counts=_poisoned(4 * users, torch.int64, dev), cws=_poisoned(size_of(C.cast(vd, C.c_void_p), n), torch.uint8, dev),
               ws=_poisoned(lib.sumk_eval_device_select_long_workspace_bytes(n, max(q.n_segs for q in sd), max(q.capacity for q in sd)), torch.uint8, dev))

    def enqueue():
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        host = C.cast(vd, C.c_void_p)
        _lib.check(lib.sumk_eval_device_segments_long(scores.data_ptr(), vd_dev.data_ptr(), host, n, out["scratch"].data_ptr(), seg.data_ptr(), st), "segments_long")
        if kendall:
            _lib.check(lib.sumk_eval_device_kendall_long(scores.data_ptr(), vd_dev.data_ptr(), host, kd_dev.data_ptr(), n, out["cws"].data_ptr(), out["cws"].numel(),
                                                         out["corr"].data_ptr(), out["counts"].data_ptr(), st), "kendall_long")
        else:
            _lib.check(lib.sumk_eval_device_spearman_long(scores.data_ptr(), vd_dev.data_ptr(), host, n, out["cws"].data_ptr(), out["cws"].numel(),
                                                          out["corr"].data_ptr(), st), "spearman_long")
        _lib.check(lib.sumk_eval_device_select_long(sd_dev.data_ptr(), C.cast(sd, C.c_void_p), n, out["summary"].data_ptr(), total, out["selected"].data_ptr(), segs,
                                                    out["f"].data_ptr(), out["f"].data_ptr() + 8 * n, out["status"].data_ptr(), out["ws"].data_ptr(),
                                                    out["ws"].numel(), st), "select_long")

    def snapshot():
        torch.cuda.synchronize(dev)
        return {k: out[k].cpu().numpy().copy() for k in ("corr", "f", "status", "summary", "selected") + (("counts",) if kendall else ())}

    def poison():
        for t in out.values():
            t.view(torch.uint8).fill_(255)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                    # one capture stream, the launches in order: a linear graph
        enqueue()
    rng = np.random.default_rng(64)
    for rep in range(2):
        s = [(rng.integers(-2, 15, size=T) / 16.0).astype(np.float32) for T in lens]
        scores.copy_(torch.from_numpy(np.concatenate(s)).to(dev))
        poison()
        enqueue()
        eager = snapshot()
        poison()
        g.replay()
        replayed = snapshot()
        for k in eager:
            np.testing.assert_array_equal(replayed[k].view(np.uint8), eager[k].view(np.uint8), err_msg=f"{k}, replay {rep}")
        assert eager["status"].tolist() == [0, 0, 0]
        want = eval_native.evaluate_batch(vids, s, 0.15, "knapsack", want_summaries=True, metric=metric, n_threads=2)
        np.testing.assert_array_equal(eager["f"][:n], want[1]); np.testing.assert_array_equal(eager["summary"], np.concatenate(want[3]))
        if kendall:
            np.testing.assert_array_equal(eager["corr"], want[0])
        else:
            np.testing.assert_allclose(eager["corr"], want[0], rtol=0, atol=1e-12)
