"""CPU: SumGAN-Att's model classes (summarizer_amd.models.sumgan_att) build the reference's parameters -- same state_dict keys, shapes
and seeded initial weights (bit for bit, by sha256) as the reference modules (tests/golden/sumgan_att.npz) -- and the reference alias for it is opt-in."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden

REF = "/root/reference"


def _model(g):
    from summarizer_amd.models.sumgan_att import SumGANAtt
    D, heads, layers, seed = (int(v) for v in g["meta"])
    torch.manual_seed(seed)
    return SumGANAtt(input_size=D, s_encoder_layers=layers, s_attention_heads=heads, ae_encoder_layers=layers,
                     ae_attention_heads=heads, cLSTM_hidden_size=32, cLSTM_num_layers=layers)


def test_state_dict_matches_reference_initial_weights():
    g = load_golden("sumgan_att")
    import recipes as R
    sd = _model(g).state_dict()
    keys = [str(k) for k in g["w0keys"]]
    assert sorted(sd) == sorted(keys)
    for k, shape, sha in zip(keys, g["w0shape"], g["w0sha"]):
        assert tuple(sd[k].shape) == tuple(int(d) for d in shape if d >= 0), k
        assert R.digest({k: sd[k].numpy()}) == sha, k          # sha256 of the exact fp32 bytes


def test_selector_norm_is_shared():
    g = load_golden("sumgan_att")
    sel = _model(g).summarizer.selector
    assert sel.transformer_encoder.norm is sel.layer_norm


def test_forward_refuses_cpu_tensors():
    from summarizer_amd._lib import SumkError
    g = load_golden("sumgan_att")
    m = _model(g).eval()
    with torch.no_grad(), pytest.raises(SumkError):
        m(torch.from_numpy(g["T17/x"]))


def test_default_aliases_unchanged():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import summarizer_amd; a = summarizer_amd.install_as_reference(); "
            "print(len(a), 'summarizer.models.sumgan_att' in sys.modules)")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["6", "False"]


def test_unknown_opt_in_is_refused():
    import summarizer_amd
    with pytest.raises(ValueError):
        summarizer_amd.install_as_reference(opt_in=("rand",))


SCRIPT = r'''
import os, sys, types
root, ref = sys.argv[1:3]
sys.path.insert(0, root); sys.path.append(ref)
sys.dont_write_bytecode = True
sys.modules["h5py"] = types.ModuleType("h5py")
tb = types.ModuleType("torch.utils.tensorboard")
class SummaryWriter:
    def __init__(self, *a, **k): pass
tb.SummaryWriter = SummaryWriter
sys.modules["torch.utils.tensorboard"] = tb
import summarizer_amd
installed = summarizer_amd.install_as_reference(opt_in=("sumgan_att",))
import summarizer.utils.config as cfg                     # the reference's file, unedited: its `-m sumgan_att` registry entry
print(len(installed), cfg.SumGANAttTrainer.__module__, cfg.SumGANAttTrainer.__name__)
'''


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "summarizer")), reason="reference checkout not present")
def test_opt_in_alias_resolves_reference_config():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split()[-3:] == ["7", "summarizer_amd.models.sumgan_att", "SumGANAttTrainer"], r.stdout


# ------------------------------------------------------------------------------------------------ the float64 stack references
# oracle/torch_port.tf_encoder_stack_ref / tf_decoder_stack_ref (the oracles of tests/test_gpu_sumgan_att_f64.py) against torch's own
# nn.TransformerEncoder / nn.TransformerDecoder in float64, and recipes.tf_stack_drop_masks against transformer_drop_masks.
LENS_REF = [1, 5, 9]
D_REF, L_REF = 32, 2
REL_REF = 1e-12


def _stock(kind, heads, F_, seed, norm=False):
    import torch.nn as nn
    torch.manual_seed(seed)
    if kind == "decoder":
        m = nn.TransformerDecoder(nn.TransformerDecoderLayer(d_model=D_REF, nhead=heads, dim_feedforward=F_, dropout=0.0), num_layers=L_REF)
    else:
        m = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=D_REF, nhead=heads, dim_feedforward=F_, dropout=0.0), num_layers=L_REF,
                                  norm=nn.LayerNorm(D_REF) if norm else None, enable_nested_tensor=False)
    m = m.double()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():           # biases start at 0 and norm gains at 1 in torch: move them all
            if n.endswith("bias") or "norm" in n:
                p.add_(0.2 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    return m


def _stack_inputs(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(sum(LENS_REF), D_REF, generator=g, dtype=torch.float64) for _ in range(n)]


def _stock_run(m, ins, G):
    """Per video through the stock module (T, 1, D): loss = sum(out * G) -> out, input grads, {name: grad}"""
    for p in m.parameters():
        p.grad = None
    xs = [t.clone().requires_grad_(True) for t in ins]
    out, r0 = [], 0
    for T in LENS_REF:
        out.append(m(*[x[r0:r0 + T].unsqueeze(1) for x in xs]).squeeze(1))
        r0 += T
    out = torch.cat(out)
    (out * G).sum().backward()
    return out.detach(), [x.grad for x in xs], {n: p.grad.clone() for n, p in m.named_parameters()}


def _ref_run(kind, m, heads, ins, G, masks=None, norm=False):
    from oracle import torch_port
    p = {n: q.detach().clone().requires_grad_(True) for n, q in m.named_parameters()}
    xs = [[v.clone().requires_grad_(True) for v in torch.split(t, LENS_REF)] for t in ins]
    if kind == "decoder":
        out = torch_port.tf_decoder_stack_ref(xs[0], xs[1], p, "layers.", L_REF, heads, 1e-5, masks=masks)
    else:
        out = torch_port.tf_encoder_stack_ref(xs[0], p, "layers.", L_REF, heads, 1e-5, final_norm="norm." if norm else None, final_eps=1e-5,
                                              masks=masks)
    (out * G).sum().backward()
    return out.detach(), [torch.cat([v.grad for v in vs]) for vs in xs], {n: q.grad for n, q in p.items()}


def _close(a, b, what):
    if float(b.norm()) == 0.0:                      # (a gradient through a zeroed block: exactly zero on both sides)
        assert float(a.norm()) == 0.0, what
        return
    err = float((a - b).norm() / b.norm())
    assert err <= REL_REF, (what, err)


def _same_results(got, want, what):
    _close(got[0], want[0], what + " forward")
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        _close(a, b, f"{what} input grad {i}")
    assert set(got[2]) == set(want[2])
    for n in want[2]:
        _close(got[2][n], want[2][n], f"{what} {n}")


@pytest.mark.parametrize("F_", [D_REF, 2 * D_REF], ids=["F=D", "F=2D"])
@pytest.mark.parametrize("heads", [1, 4])
def test_decoder_stack_ref_equals_stock_decoder(heads, F_):
    m = _stock("decoder", heads, F_, 100 + heads)
    tgt, mem, G = _stack_inputs(5, 3)
    _same_results(_ref_run("decoder", m, heads, [tgt, mem], G), _stock_run(m, [tgt, mem], G), f"decoder heads={heads} F={F_}")


@pytest.mark.parametrize("norm", [True, False], ids=["final_norm", "no_norm"])
@pytest.mark.parametrize("F_", [D_REF, 2 * D_REF], ids=["F=D", "F=2D"])
@pytest.mark.parametrize("heads", [1, 4])
def test_encoder_stack_ref_equals_stock_encoder(heads, F_, norm):
    m = _stock("encoder", heads, F_, 200 + heads, norm)
    x, G = _stack_inputs(6, 2)
    _same_results(_ref_run("encoder", m, heads, [x], G, norm=norm), _stock_run(m, [x], G), f"encoder heads={heads} F={F_} norm={norm}")


def _ones_masks(heads, F_, decoder):
    R_ = sum(LENS_REF)
    one = lambda *s: torch.ones(*s, dtype=torch.float64)
    mk = {"attn": [[one(heads, T, T) for T in LENS_REF] for _ in range(L_REF)], "out": [one(R_, D_REF) for _ in range(L_REF)],
          "ff1": [one(R_, F_) for _ in range(L_REF)], "ff2": [one(R_, D_REF) for _ in range(L_REF)]}
    if decoder:
        mk.update(cattn=[[one(heads, T, T) for T in LENS_REF] for _ in range(L_REF)], cout=[one(R_, D_REF) for _ in range(L_REF)])
    return mk


@pytest.mark.parametrize("kind", ["decoder", "encoder"])
def test_all_ones_masks_change_no_bit(kind):
    heads, F_ = 4, 2 * D_REF
    m = _stock(kind, heads, F_, 300)
    ins = _stack_inputs(7, 3 if kind == "decoder" else 2)
    a = _ref_run(kind, m, heads, ins[:-1], ins[-1])
    b = _ref_run(kind, m, heads, ins[:-1], ins[-1], masks=_ones_masks(heads, F_, kind == "decoder"))
    assert torch.equal(a[0], b[0]) and all(torch.equal(u, v) for u, v in zip(a[1], b[1]))
    assert all(torch.equal(a[2][n], b[2][n]) for n in a[2])


@pytest.mark.parametrize("site", ["cattn", "cout"])
def test_zeroed_decoder_site_removes_that_sub_block(site):
    """Layer 1's cross-attention with one whole site masked to zero, against the stock decoder with that contribution removed:
    "cout" = 0 leaves norm2(h + 0), i.e. a zero out-projection (weight and bias); "cattn" = 0 leaves a zero context, so the
    out-projection passes its bias only, i.e. a zero V projection (rows [2D, 3D) of in_proj, weight and bias)."""
    import copy
    heads, F_, l = 4, 2 * D_REF, 1
    m = _stock("decoder", heads, F_, 400)
    tgt, mem, G = _stack_inputs(8, 3)
    masks = _ones_masks(heads, F_, True)
    masks[site][l] = [torch.zeros_like(a) for a in masks[site][l]] if site == "cattn" else torch.zeros_like(masks[site][l])
    got = _ref_run("decoder", m, heads, [tgt, mem], G, masks=masks)
    cut = copy.deepcopy(m)
    ca = cut.layers[l].multihead_attn
    with torch.no_grad():
        if site == "cout":
            ca.out_proj.weight.zero_(); ca.out_proj.bias.zero_()
        else:
            ca.in_proj_weight[2 * D_REF:].zero_(); ca.in_proj_bias[2 * D_REF:].zero_()
    want = _stock_run(cut, [tgt, mem], G)
    full = _stock_run(m, [tgt, mem], G)
    assert float((want[0] - full[0]).abs().max()) > 1e-3          # the removed block did contribute
    _close(got[0], want[0], site + " forward")
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        _close(a, b, f"{site} input grad {i}")
    zeroed = ("multihead_attn.out_proj.", "multihead_attn.in_proj_") if site == "cout" else ("multihead_attn.in_proj_",)
    for n in want[2]:
        if n.startswith(f"layers.{l}.") and any(z in n for z in zeroed):
            continue                                              # parameters of the removed block itself: other functions of them
        _close(got[2][n], want[2][n], f"{site} {n}")


def test_tf_stack_drop_masks():
    import numpy as np
    import recipes as R
    seed, p, lens, D, F_, heads, L = 0xABCDEF, 0.1, [1, 5, 70], 32, 48, 4, 2
    R_ = sum(lens)
    enc = R.tf_stack_drop_masks(seed, p, lens, D, F_, heads, L, decoder=False)
    dec = R.tf_stack_drop_masks(seed, p, lens, D, F_, heads, L, decoder=True)
    old = R.transformer_drop_masks(seed, p, 0.5, lens, D, F_, heads, L)
    assert set(enc) == {"attn", "out", "ff1", "ff2"} and set(dec) == set(enc) | {"cattn", "cout"}
    kept = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    for mk in (enc, dec):
        for k, v in mk.items():
            assert len(v) == L
            for l in range(L):
                if k in ("attn", "cattn"):
                    assert [a.shape for a in v[l]] == [(heads, T, T) for T in lens]
                    arrs = v[l]
                else:
                    assert v[l].shape == (R_, F_ if k == "ff1" else D)
                    arrs = [v[l]]
                for a in arrs:
                    assert a.dtype == np.float32 and set(np.unique(a)) <= {np.float32(0), kept}
        for k in ("out", "ff1", "ff2"):
            assert all(np.array_equal(mk[k][l], old[k][l]) for l in range(L)), k
        assert all(np.array_equal(a, b) for l in range(L) for a, b in zip(mk["attn"][l], old["attn"][l]))
    for l in range(L):                                            # sites +4 / +5 are draws of their own
        assert not np.array_equal(dec["cout"][l], dec["out"][l]) and not np.array_equal(dec["cout"][l], dec["ff2"][l])
        assert not np.array_equal(dec["cattn"][l][2], dec["attn"][l][2])
        assert abs(float((dec["cout"][l] > 0).mean()) - 0.9) < 0.03 and abs(float((dec["cattn"][l][2] > 0).mean()) - 0.9) < 0.03
    assert not np.array_equal(dec["cout"][0], dec["cout"][1]) and not np.array_equal(dec["cattn"][0][2], dec["cattn"][1][2])
