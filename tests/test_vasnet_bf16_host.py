"""CPU only: the reference and the gates of tests/test_gpu_vasnet_bf16_f64.py can tell right from wrong.  The float64 emulation of the bf16
training step (tests/vasnet_bf16_common.py: E64, its reference-only ensemble, relative L2 per tensor and per video) at D = 256 on two small
ragged batches.  Five seeded faults are applied to the emulated port alone; each must stand out against the yardstick on at least one
tensor by err / yardstick >= 4 x MULT (four times over its gate) -- the printed ratios are what caps MULT (a quarter of the smallest).
The helper itself is guarded: every ensemble member is within its own yardstick, bf16-representable inputs pass the leaf rounding
unchanged, and the dispatch restated in `regime` puts every GPU case on the path it is named for."""
import numpy as np
import pytest
import torch

import vasnet_bf16_common as B

D = 256
LENS = {"a": [321, 130, 47], "b": [1025, 600, 3]}
P = 0.5


@pytest.fixture(scope="module")
def model():
    torch.set_num_threads(8)
    return B.make_params(D)


_WORLD = {}


def world(model, case, mask, p=P):
    """E64, its ensemble and yardstick for (case, mask): computed once per module."""
    key = (case, mask, p)
    if key not in _WORLD:
        params, scale, eps = model
        lens = LENS[case]
        x, w = B.make_batch(lens, D)
        masks = B.drop_masks(lens, D, p)
        ref, members = B.ensemble(params, x, w, lens, scale, eps, torch.device("cpu"), mask, masks)
        _WORLD[key] = dict(lens=lens, x=x, w=w, masks=masks, ref=ref, members=members, yard=B.yardstick(ref, members, lens))
    return _WORLD[key]


def _faulty(model, wd, mask, fault):
    params, scale, eps = model
    return B.port_step(params, wd["x"], wd["w"], wd["lens"], scale, eps, torch.float64, torch.device("cpu"), mask, wd["masks"], fault=fault)


FAULTS = {
    # name: (case, mask, fault)
    "last_key_of_a_video_masked": ("a", "plain", dict(drop_key=(0, 320))),
    "first_key_of_a_k_tile_masked": ("b", "plain", dict(drop_key=(1, 576))),          # key 64 x 9 of the 600-frame video
    "aperture_off_by_one": ("a", "band64", dict(aperture_delta=1)),
    "ignore_self_not_applied": ("a", "noself", dict(no_ignore_self=True)),
    "alpha_mask_by_video_local_row": ("b", "plain", dict(alpha_local_rows=1, p=P)),
}


@pytest.mark.parametrize("name", list(FAULTS))
def test_seeded_fault_stands_out(model, name):
    case, mask, fault = FAULTS[name]
    wd = world(model, case, mask)
    rec, bad = B.judge(f"host/{name}", _faulty(model, wd, mask, fault), wd["ref"], wd["yard"], wd["lens"], quiet=True)
    t = rec["tensors"][rec["worst"]]
    print(f"\nBF16-HOST fault {name}: err / yardstick {rec['worst_ratio']:.4g} on {rec['worst']} (err {t['err']:.3e}, yardstick "
          f"{t['yardstick']:.3e}, err / gate {t['err'] / t['gate']:.4g}); tensors over their gate: {len(bad)}")
    assert bad, name
    assert rec["worst_ratio"] >= 4 * B.MULT, (name, rec["worst"], rec["worst_ratio"])


@pytest.mark.parametrize("case,mask", [("a", "plain"), ("b", "plain"), ("a", "band64"), ("a", "noself")])
def test_ensemble_members_stay_within_the_yardstick(model, case, mask):
    wd = world(model, case, mask)
    ref = wd["ref"]
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    s = torch.sigmoid(ref["logits"])
    assert float(s.min()) > 0.01 and float(s.max()) < 0.99, (float(s.min()), float(s.max()))          # logits recoverable from fp32 scores
    assert all(y > 0 for y in wd["yard"].values()), [k for k, y in wd["yard"].items() if not y > 0]
    for m in wd["members"]:
        rec, bad = B.judge("host/member", m, ref, wd["yard"], wd["lens"], quiet=True)
        assert not bad and rec["worst_ratio"] <= 1.0, (rec["worst"], rec["worst_ratio"])
    B.REPORT.clear()


def test_unfaulted_port_is_the_reference(model):
    wd = world(model, "a", "plain")
    got = _faulty(model, wd, "plain", {})
    assert all(torch.equal(got[k], wd["ref"][k]) for k in got)


def test_leaf_rounding_leaves_bf16_values_alone(model):
    """x and the weight matrices already bf16 values: E64 with the leaf rounding skipped is bit-identical to E64 with it (the fp32 -> bf16
    step of the float64 port is idempotent and rounds nothing it should not)."""
    params, scale, eps = model
    lens = LENS["a"]
    x, w = B.make_batch(lens, D)
    r16 = lambda t: t.to(torch.bfloat16).to(torch.float32)
    pr = {k: r16(v) if k in B.MATS else v for k, v in params.items()}
    masks = B.drop_masks(lens, D, P)
    a, b = (B.port_step(pr, r16(x), w, lens, scale, eps, torch.float64, torch.device("cpu"), "plain", masks, round_leaves=rl) for rl in (True, False))
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = B.port_step(params, x, w, lens, scale, eps, torch.float64, torch.device("cpu"), "plain", masks, round_leaves=False)
    assert not torch.equal(a["dX"], c["dX"])          # (and on fp32 inputs the leaf rounding does something)


def test_nudge_moves_every_element_by_one_ulp():
    t = torch.tensor([1.0, -1.0, 0.0, 3.5e-5, 1e30], dtype=torch.float32).repeat(100)
    n = B.nudge(t, 3)
    steps = (n.view(torch.int32).long() - t.view(torch.int32).long()).abs()
    assert bool(((steps == 1) | (t == 0)).all()) and bool((n != t).all())
    assert 0.2 < float((n > t).float().mean()) < 0.8


def test_every_gpu_case_reaches_its_path():
    assert B.min_rows_b16(1024) == 8065 and B.min_rows_b16(2048) == 3969
    bms = set()
    for cid, (lens, Dm, _, _) in B.CASES.items():
        g = B.check_regime(cid)
        assert g["b16"] and g["bm_qkv"] in (192, 256) and g["bm_d"] in (192, 256), (cid, g)
        bms.update((g["bm_qkv"], g["bm_d"]))
    assert bms == {192, 256}, bms                      # both wide-tile heights occur in the table
    fused = [c for c in B.CASES if B.regime(*B.CASES[c][:2])["attn_fused"]]
    assert fused == ["fused_320"], fused
    for tid, lens in B.L.TRAIN.items():
        g = B.regime(lens, B.SMALL_D)
        assert g["path"] == "inloop" and g["softmax_nr"] == {"nr4": 4, "nr8": 8, "nr16": 16}.get(tid.split("_")[0], 0), (tid, g)
    g = B.regime(B.CASES["lone_8101"][0], 1024)
    assert g["R"] % 2 == 1 and g["n_seq"] == 1
