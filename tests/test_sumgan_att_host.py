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
