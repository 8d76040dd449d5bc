"""CPU: the specification of the fused bf16 attention strips (tests/attn_strip_ref.py) pinned to oracle/torch_port's VASNet attention and to
torch autograd in float64; its dropout indices pinned to recipes.vasnet_drop_masks; the float32 specification run as the kernel through every
gate of tests/test_gpu_attn_strip.py on every family (it passes), six deliberate mistakes run the same way (each is rejected by the gate
that should catch it); the input families' own properties; the size query and the refusals of the raw entry (host arithmetic: no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_strip_cases as cases
import attn_strip_ref as ref
import recipes as R

_FWD = {}


def forward_model(name):
    """(family, float32 model of its forward), computed once."""
    if name not in _FWD:
        fam = cases.families()[name]
        _FWD[name] = (fam, [ref.model32_forward(c) for c in fam])
    return _FWD[name]


# ---------------------------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("ignore_self,aperture", [(False, -1), (True, -1), (False, 3), (True, 3)])
def test_float64_spec_matches_torch_port_and_autograd(ignore_self, aperture):
    """oracle/torch_port.vasnet_scores in float64, training dropout by recipes.vasnet_drop_masks: its scores are those of the layers behind
    the attention applied to THIS specification's context, and its autograd gradients of W_Q and W_K are dQ^T x and dK^T x of this
    specification's dS, fed with the dCTX autograd gives for that context."""
    from oracle import torch_port
    T, D, p, seed = 37, 32, 0.5, 77
    sc = float(np.float32(cases.SCALE))
    w = {k: torch.from_numpy(v.astype(np.float64)) for k, v in R.vasnet_weights(D, 5).items()}
    for k in ("Q.weight", "K.weight"):
        w[k].requires_grad_(True)
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((T, 1, D)))
    ma, my, mz = (torch.from_numpy(m.astype(np.float64))[None] for m in R.vasnet_drop_masks(seed, p, [T], D)[0])
    wl = torch.from_numpy(np.random.default_rng(7).standard_normal((T, 1, 1)))
    s_port = torch_port.vasnet_scores(x, w, ignore_self=ignore_self, aperture=None if aperture < 0 else aperture, scale=sc, drop_masks=(ma, my, mz))
    (s_port * wl).sum().backward()

    xn = x[:, 0].numpy()
    Q, K, V = (xn @ w[k].detach().numpy().T for k in ("Q.weight", "K.weight", "V.weight"))
    al = ref.alpha_spec(Q, K, [T], sc, ignore_self, aperture)[0]
    keep = ref.keep_masks([T], p, seed)[0]
    ctx = torch.from_numpy(ref.dropped(al, keep, p, np.float64) @ V).requires_grad_(True)
    ln = lambda t: torch.nn.functional.layer_norm(t, (D,), w["layer_norm.weight"], w["layer_norm.bias"], 1e-6)
    y = ln((ctx @ w["attention_head_projection.weight"].t() + x[:, 0]) * my[0])
    z = ln(torch.relu(y @ w["k1.weight"].t() + w["k1.bias"]) * mz[0])
    s = torch.sigmoid(z @ w["k2.weight"].t() + w["k2.bias"])
    assert (s - s_port[:, 0]).abs().max().item() <= 1e-12
    (s * wl[:, 0]).sum().backward()
    ds = ref.ds_spec(ctx.grad.numpy(), V, al, keep, p, sc)
    for name, g in (("Q.weight", (ds @ K).T @ xn), ("K.weight", (ds.T @ Q).T @ xn)):
        want = w[name].grad.numpy()
        assert np.abs(want).max() > 1e-6 and np.abs(g - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), name


def test_dropout_indices_match_the_recipes():
    lens, p, seed, D = (5, 1, 66, 130), 0.3, 1234, 8
    for keep, (m_alpha, _, _) in zip(ref.keep_masks(lens, p, seed), R.vasnet_drop_masks(seed, p, lens, D)):
        assert np.array_equal(keep.astype(np.float32) * ref.drop_scale(p), m_alpha)
    assert 0.2 < 1.0 - np.concatenate([k.ravel() for k in ref.keep_masks(lens, p, seed)]).mean() < 0.4
    assert not np.array_equal(ref.keep_masks((66,), 0.5, 1)[0], ref.keep_masks((66,), 0.5, 2)[0])
    # rows are those of the PACKED batch: the second video's mask is not the mask of a video that starts at row 0
    assert not np.array_equal(ref.keep_masks((5, 66), 0.5, 1)[1], ref.keep_masks((66,), 0.5, 1)[0])
    assert all(k.all() for k in ref.keep_masks(lens, 0.0, seed))


def test_bf16_helpers_match_torch():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 4000).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, np.inf, -np.inf, 3.4e38, 1e-40, 65280.0], np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(ref.bf16_bits(x), want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(ref.bf16_value(ref.bf16_bits(x)), want.float().numpy())
    assert np.isnan(ref.bf16_value(ref.bf16_bits(np.array([np.nan], np.float32)))).all()
    for v, hs in ((1.0, 2.0 ** -8), (1.99, 2.0 ** -8), (2.0, 2.0 ** -7), (0.75, 2.0 ** -9), (0.0, 2.0 ** -134), (-3.0, 2.0 ** -7)):
        assert ref.bf16_half_spacing(v) == hs, v


# ---------------------------------------------------------------------------------------------------------------- the families
def test_case_families_are_what_the_gpu_test_relies_on():
    fams = cases.families()
    assert [c["lens"][0] for c in fams["edges"]] == list(cases.EDGE_T) and all(c["D"] == 256 and len(c["lens"]) == 1 for c in fams["edges"])
    assert {(T + 63) // 64 for T in cases.EDGE_T} == {1, 2, 3, 4, 5}
    assert [len(c["lens"]) for c in fams["ragged"]] == [1, 7, 8, 9, 17]
    assert all(c["p"] == 0.5 and c["D"] == 256 and 1 <= min(c["lens"]) and max(c["lens"]) <= 320 for c in fams["ragged"])
    assert all(1 in c["lens"] and 320 in c["lens"] for c in fams["ragged"][1:])
    assert [c["D"] for c in fams["width"]] == [512, 1024, 2048] and all(c["lens"] == [65, 3, 320] and c["p"] == 0.5 for c in fams["width"])
    assert sorted({c["p"] for c in fams["dropout"]}) == [0.0, 0.1, 0.5, 0.9]
    for fam in fams.values():
        for c in fam:
            for n in ("q", "k", "v", "dctx"):
                assert c[n].dtype == np.float32 and np.array_equal(ref.bf16_round(c[n]), c[n]), (c["name"], n)       # bf16 values
            assert c["scale"] == cases.SCALE
    # masks: every rule, and the underflow clause of the mask rule is not in play (no in-band |logit * scale| below 1e-15)
    seen = {(c["ignore_self"], c["aperture"]) for c in fams["masks"]}
    assert seen == {(True, -1), (False, 0), (True, 0), (False, 3), (True, 3), (False, 400), (True, 400)}
    for c in fams["masks"]:
        for r0, T in ref.videos(c["lens"]):
            e = np.abs(c["q"][r0:r0 + T].astype(np.float64) @ c["k"][r0:r0 + T].astype(np.float64).T * cases.SCALE)
            assert e.min() >= 1e-15, c["name"]
        nan_rows = [np.isnan(a).all(axis=1) for a in ref.alpha_spec(c["q"], c["k"], c["lens"], c["scale"], c["ignore_self"], c["aperture"])]
        if c["forward_only"]:
            assert any(r.any() for r in nan_rows), c["name"]           # forward only BECAUSE a row has no key left
        else:
            assert not any(r.any() for r in nan_rows), c["name"]
    assert any(c["lens"] == [1] and c["ignore_self"] for c in fams["masks"])


def test_loud_rows_are_loud():
    c, = cases.loud()
    a32 = np.zeros((sum(c["lens"]), max(c["lens"])), dtype=np.float32)
    e64 = np.zeros_like(a32, dtype=np.float64)
    for (r0, T), a in zip(ref.videos(c["lens"]), ref.alpha_spec(c["q"], c["k"], c["lens"], c["scale"], dtype=np.float32)):
        a32[r0:r0 + T, :T] = a
        e64[r0:r0 + T, :T] = c["q"][r0:r0 + T].astype(np.float64) @ c["k"][r0:r0 + T].astype(np.float64).T * cases.SCALE
    for r in c["saturating_rows"]:
        key = c["loud_keys"][0] if r < c["lens"][0] else c["loud_keys"][1] - c["lens"][0]
        assert a32[r, key] == 1.0 and a32[r].sum() == 1.0 and 35.0 < e64[r, key] < 45.0, r            # one key at +40, the rest exactly 0
    for rows, off in ((c["offset30_rows"], 30.0), (c["offset100_rows"], 100.0)):
        for r in rows:
            T = c["lens"][0] if r < c["lens"][0] else c["lens"][1]
            assert abs(np.median(e64[r, :T]) - off) < 1.0 and e64[r, :T].min() > off - 6.0, r
    assert all(e64[r].max() > 88.8 for r in c["offset100_rows"])                                      # exp overflows float32 without the row maximum


# ---------------------------------------------------------------------------------------------------------------- the gates
@pytest.mark.parametrize("name", ["edges", "ragged", "masks", "width", "loud", "dropout"])
def test_float32_spec_passes_every_gate(name):
    fam, outs = forward_model(name)
    r = ref.check_forward(fam, outs)
    assert r["E"][0] <= 1.0 + 1e-9 and r["O16"][0] <= 1.0 + 1e-9, r        # by construction: the model IS the yardstick
    both = [(c, o) for c, o in zip(fam, outs) if not c["forward_only"]]
    bfam, Es = [c for c, _ in both], [o["E"] for _, o in both]
    r = ref.check_backward(bfam, Es, [ref.model32_backward(c, E) for c, E in zip(bfam, Es)])
    assert r["dS"][0] <= 1.0 + 1e-9 and r["dQ"][0] <= 1.0 + 1e-9, r


def _pick(name, keep):
    fam, outs = forward_model(name)
    idx = [i for i, c in enumerate(fam) if keep(c)]
    assert idx
    return [fam[i] for i in idx], [outs[i] for i in idx]


MUTANT_CASES = {
    # mutant: (family, case filter, the gate that must reject it)
    "drop_last_key_tile": ("edges", lambda c: c["lens"][0] in (33, 65, 96, 129, 320), r"\('E', .*elements outside the gate"),
    "swap_p_chunks": ("edges", lambda c: c["lens"][0] in (33, 129, 320), r"\('O16', .*elements outside the gate"),
    "local_dropout_row": ("ragged", lambda c: len(c["lens"]) == 7, r"P16 differs from bf16_rne"),
    "no_max_subtraction": ("loud", lambda c: True, r"\('E', .*NaN positions differ"),
    "pad_column_nonzero": ("edges", lambda c: c["lens"][0] in (33, 65, 319), r"P16 pad columns are not exactly 0"),
    "bf16_truncation": ("dropout", lambda c: c["p"] in (0.0, 0.5), r"P16 differs from bf16_rne"),
}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_gates_reject_the_mutant(mutant):
    name, keep, why = MUTANT_CASES[mutant]
    fam, outs = _pick(name, keep)
    ref.check_forward(fam, outs)                                            # the same cases pass unmutated ...
    for i in range(len(fam)):                                               # ... and ONE mutated case among them is enough to fail
        mut = list(outs)
        mut[i] = ref.model32_forward(fam[i], mutant)
        with pytest.raises(AssertionError, match=why):
            ref.check_forward(fam, mut)


def test_swapped_chunks_fail_on_most_of_the_row():
    """Two 8-key chunks of one P row swapped before the second product: at T = 320, D = 256 nearly all of that row's 256 CTX elements
    leave the gate (the few that stay are columns where the two chunks' contributions happen to be close)."""
    fam, outs = _pick("edges", lambda c: c["lens"][0] == 320)
    with pytest.raises(AssertionError) as ei:
        ref.check_forward(fam, [ref.model32_forward(fam[0], "swap_p_chunks")])
    assert ei.value.args[0][0] == "O16" and ei.value.args[0][3] > 240, ei.value.args[0]


def test_backward_gates_reject_a_local_dropout_row_and_truncation():
    fam, outs = _pick("ragged", lambda c: len(c["lens"]) == 7)
    Es = [o["E"] for o in outs]
    with pytest.raises(AssertionError, match=r"\('dS', .*elements outside the gate"):
        ref.check_backward(fam, Es, [ref.model32_backward(fam[0], Es[0], "local_dropout_row")])
    # the forward's mask read back from its P16 (P16 == 0 where E != 0) is the specification's mask
    c, o = fam[0], outs[0]
    back = [~((P[:, :T] == 0) & (E[:, :T] != 0)) for (r0, T), E, P in zip(ref.videos(c["lens"]), o["E"], o["P16"])]
    spec = ref.keep_masks(c["lens"], c["p"], c["seed"])
    assert all(np.array_equal(b | (E[:, :b.shape[1]] == 0), s | (E[:, :b.shape[1]] == 0)) for b, s, E in zip(back, spec, o["E"]))
    ref.check_backward(fam, Es, [ref.model32_backward(c, Es[0])], keeps=[back])


# ---------------------------------------------------------------------------------------------------------------- the raw entry on the host
@pytest.fixture(scope="module")
def lib():
    from summarizer_amd import _lib
    return _lib.load()


def _off(lens):
    return (C.c_int32 * (len(lens) + 1))(0, *np.cumsum(lens).tolist())


def test_size_query_on_the_host(lib):
    e, p = C.c_int64(-1), C.c_int64(-1)
    for lens in ((1,), (320,), (65, 3, 320), tuple(cases.ragged_lens(17))):
        assert lib.sumk_attn_strips_b16_sizes(len(lens), _off(lens), C.byref(e), C.byref(p)) == 0, lib.sumk_last_error()
        assert (e.value, p.value) == ref.sizes(lens), lens
    assert ref.sizes((65, 3, 320)) == (65 * 68 + 3 * 4 + 320 * 320, 65 * 128 + 3 * 64 + 320 * 320)
    assert lib.sumk_attn_strips_b16_sizes(2, _off((5, 0)), C.byref(e), C.byref(p)) == -1 and b"video 1 has 0 frames" in lib.sumk_last_error()
    assert lib.sumk_attn_strips_b16_sizes(0, _off(()), C.byref(e), C.byref(p)) == -1 and b"n_seq" in lib.sumk_last_error()
    assert lib.sumk_attn_strips_b16_sizes(1, None, C.byref(e), C.byref(p)) == -1 and b"seq_off_host" in lib.sumk_last_error()
    assert lib.sumk_attn_strips_b16_sizes(1, _off((5,)), None, C.byref(p)) == -1 and b"e_elems" in lib.sumk_last_error()


def test_raw_entry_refusals_on_the_host(lib):
    """Every refusal comes before the first device call, so it is host arithmetic: the pointers are never followed."""
    PTR = 0x7000000000

    def call(msg, lens=(10,), D=256, lda=256, ldb=256, ldc=256, ldo=256, p=0.0, **ptrs):
        a = dict(A16=PTR, B16=PTR, C16=PTR, O16=PTR, E=PTR, P16=PTR)
        a.update(ptrs)
        off = _off(lens) if lens is not None else None
        rc = lib.sumk_attn_strips_b16(0, a["A16"], lda, a["B16"], ldb, a["C16"], ldc, a["O16"], ldo, a["E"], a["P16"], D, len(lens or (1,)), off,
                                      0.06, 0, -1, p, 1, None)
        assert rc == -1 and msg in lib.sumk_last_error(), (rc, msg, lib.sumk_last_error())

    for name in ("A16", "B16", "C16", "O16", "E", "P16"):
        call(name.encode() + b" is null", **{name: None})
    call(b"seq_off_host is null", lens=None)
    call(b"video 1 has 0 frames", lens=(10, 0, 5))
    call(b"not eligible (t_max=321", lens=(321,))
    call(b"not eligible", D=128, lda=128, ldb=128, ldc=128, ldo=128)
    call(b"not eligible", D=384, lda=384, ldb=384, ldc=384, ldo=384)
    call(b"not eligible", lens=(320,), lda=1 << 22, ldb=1 << 22, ldc=1 << 22)           # byte offsets past 31 bits
    for ld in ("lda", "ldb", "ldc", "ldo"):
        call(ld.encode() + b"=248 must be at least D=256", **{ld: 248})
        call(ld.encode() + b"=260 must be at least D=256 and a multiple of 8", **{ld: 260})
    for name, ld in (("A16", b"lda"), ("B16", b"ldb"), ("C16", b"ldc"), ("O16", b"ldo")):
        call(b"the operand of " + ld + b" is not 16-byte aligned", **{name: PTR + 8})
    call(b"E is not 16-byte aligned", E=PTR + 4)
    call(b"P16 is not 16-byte aligned", P16=PTR + 2)
    call(b"dropout_p=1 must lie in [0, 1)", p=1.0)
    call(b"must lie in [0, 1)", p=-0.5)


def test_wrapper_has_no_cpu_fallback():
    from summarizer_amd import kernels
    from summarizer_amd._lib import SumkError
    sb = kernels.SeqBatch([10], "cpu")
    t = torch.zeros(10, 256, dtype=torch.bfloat16)
    with pytest.raises(SumkError, match="must be a GPU bfloat16"):
        kernels.attn_strips_b16(False, t, t, t, t.clone(), torch.zeros(120), torch.zeros(640, dtype=torch.bfloat16), sb, 0.06)
    assert kernels.attn_strips_b16_sizes(sb) == (10 * 12, 10 * 64)
