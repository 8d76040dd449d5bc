#!/usr/bin/env python3
"""Goldens for SumGAN-Att from the REAL reference modules (summarizer/models/sumgan_att.py; small model: D = 64, 4 heads, 2 + 2 + 2
layers, every dropout 0): the seeded initial state_dict (shape and sha256 digest per tensor), selector scores and autoencoder x_hat of ragged videos (T = 1, 17, 40), and the
decoder stack's output for given tgt / memory.  -> tests/golden/sumgan_att.npz.  Run once in the build container:
   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sumgan_att.py"""
import os, sys, types
import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"; sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
for name in ["h5py", "ortools", "ortools.algorithms", "ortools.algorithms.pywrapknapsack_solver"]:
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["ortools.algorithms"].pywrapknapsack_solver = sys.modules["ortools.algorithms.pywrapknapsack_solver"]
sys.path.insert(0, "/root/reference")
import torch
import summarizer.models.sumgan_att as ref
sys.path.insert(0, HERE)
import recipes as R

torch.set_num_threads(4)
D, HEADS, LAYERS, SEED, LENS = 64, 4, 2, 1234, (1, 17, 40)
out = {"meta": np.array([D, HEADS, LAYERS, SEED]), "lens": np.array(LENS)}
torch.manual_seed(SEED)
m = ref.SumGANAtt(input_size=D, s_encoder_layers=LAYERS, s_attention_heads=HEADS, ae_encoder_layers=LAYERS, ae_attention_heads=HEADS,
                  cLSTM_hidden_size=32, cLSTM_num_layers=LAYERS)
# the weights themselves are reproduced from the seed: per state_dict key its shape (padded with -1) and the sha256 of its exact
# fp32 bytes, packed into three arrays
sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
out["w0keys"] = np.array(list(sd))
out["w0shape"] = np.array([list(v.shape) + [-1] * (4 - v.ndim) for v in sd.values()], dtype=np.int64)
out["w0sha"] = np.array([R.digest({k: v}) for k, v in sd.items()])
m.eval()
rng = np.random.default_rng(5)
with torch.no_grad():
    for T in LENS:
        x = rng.standard_normal((T, 1, D)).astype(np.float32)
        out[f"T{T}/x"] = x
        out[f"T{T}/scores"] = m(torch.from_numpy(x)).numpy()
        out[f"T{T}/x_hat"] = m.summarizer.ae(torch.from_numpy(x)).numpy()
        tgt = rng.standard_normal((T, 1, D)).astype(np.float32)
        mem = rng.standard_normal((T, 1, D)).astype(np.float32)
        out[f"T{T}/tgt"], out[f"T{T}/mem"] = tgt, mem
        out[f"T{T}/dec"] = m.summarizer.ae.transformer_decoder(torch.from_numpy(tgt), torch.from_numpy(mem)).numpy()
np.savez_compressed(os.path.join(HERE, "sumgan_att.npz"), **out)
print("wrote", len(out), "arrays")
