#!/usr/bin/env python3
"""End-to-end golden from the REAL reference SumGANAttTrainer (autoencoder pre-training, then selector+encoder / decoder /
discriminator updates with three Adam optimisers; supervised sparsity, input noise in epoch 0), small model (D = 64, 4 heads,
2 + 2 + 2 layers), synthetic SumMe-shaped dataset, in-memory h5py stand-in, every dropout of the model set to 0 after reset().
Weights are stored compactly: the initial ones as sha256 digests, the final ones at 256 seeded sample indices per tensor (as train_full.npz).
torch.randn_like / torch.rand (uniform scores, noise) are replaced by recipes.DetRandom so the HIP trainer can be fed the same draws.
-> tests/golden/e2e_sumgan_att.npz.   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_e2e_sumgan_att.py"""
import os, sys, types, random
import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"; sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
from summarizer_amd.utils.datasets import synthetic_dataset
from summarizer_amd.utils.hps import make_hps
import recipes as R

DS = {}
h5 = types.ModuleType("h5py")
h5.File = lambda path, mode="r": DS[path]
sys.modules["h5py"] = h5
for name in ["ortools", "ortools.algorithms", "ortools.algorithms.pywrapknapsack_solver"]:
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["ortools.algorithms"].pywrapknapsack_solver = sys.modules["ortools.algorithms.pywrapknapsack_solver"]
sys.path.insert(0, "/root/reference")
import torch
import summarizer.models.sumgan_att as ref

torch.set_num_threads(4)
D, SEED = 64, 123
EP = {"input_size": str(D), "s_encoder_layers": "2", "s_attention_heads": "4", "ae_encoder_layers": "2", "ae_attention_heads": "4",
      "cLSTM_hidden_size": "32", "pretrain_ae": "1", "epoch_noise": "1", "sup": True}
ds = synthetic_dataset(9, seed=8, D=D, t_range=(30, 60), n_users=5)
keys = sorted(ds.keys(), key=lambda k: int(k.split("_")[1]))
DS["synthetic.h5"] = ds
hps = make_hps("synthetic.h5", [{"train_keys": keys[3:], "test_keys": keys[:3]}], epochs=2, test_every_epochs=1, lr=1e-3,
               use_cuda=False, selection_algorithm="rank", extra_params=dict(EP))
torch.manual_seed(SEED); random.seed(SEED)
tr = ref.SumGANAttTrainer(hps, hps.splits_files[0]).reset()
for mod in tr.model.modules():
    if isinstance(mod, torch.nn.Dropout):
        mod.p = 0.0
    if isinstance(mod, torch.nn.MultiheadAttention):
        mod.dropout = 0.0
w0 = {k: v.detach().numpy().copy() for k, v in tr.model.state_dict().items()}
with R.DetRandom(SEED).patch() as det:
    best = tr.train(0)
    n_draws = det.n
# initial weights: shape + sha256 of the exact fp32 bytes (the HIP trainer rebuilds them from the seed); final weights: their exact
# values at N_SAMPLE flat indices per tensor (recipes.sample_idx, seeded by the key -- the test draws the same indices)
N_SAMPLE = 256
# (packed: key k's samples are w1_sample[w1_off[i]:w1_off[i + 1]] for k = w0keys[i])
out = {"w0keys": np.array(list(w0)), "w0sha": np.array([R.digest({k: v}) for k, v in w0.items()])}
w1 = {k: v.detach().numpy().reshape(-1) for k, v in tr.model.state_dict().items()}
samples = [w1[k][R.sample_idx(k, w1[k].size, N_SAMPLE)].astype(np.float32) for k in w0]
out["w1_off"] = np.concatenate([[0], np.cumsum([len(a) for a in samples])]).astype(np.int64)
out["w1_sample"] = np.concatenate(samples)
sc = hps.writer.scalars
for t in ("Lse", "Ld", "Lc", "D_x", "D_x_hat", "D_x_hat_p"):
    out[t] = np.array([v for _, v in sc[f"synthetic/Fold_1/Train/{t}"]], dtype=np.float64)
out["corr"] = np.array([v for _, v in sc["synthetic/Fold_1/Test/Correlation"]], dtype=np.float64)
out["f_avg"] = np.array([v for _, v in sc["synthetic/Fold_1/Test/F-score_avg"]], dtype=np.float64)
out["f_max"] = np.array([v for _, v in sc["synthetic/Fold_1/Test/F-score_max"]], dtype=np.float64)
out["best"] = np.array(best, dtype=np.float64)
out["meta"] = np.array([D, SEED, 9, 8, 30, 60, 5, n_draws])
tr.model.eval()
with torch.no_grad():
    for k in keys[:3]:
        out[f"scores/{k}"] = tr.model(torch.from_numpy(ds[k]["features"][...]).unsqueeze(1)).squeeze().numpy()
np.savez_compressed(os.path.join(HERE, "e2e_sumgan_att.npz"), **out)
print({t: out[t] for t in ("Lse", "Ld", "Lc", "D_x", "D_x_hat", "D_x_hat_p", "corr", "f_avg")}, "draws", n_draws)
print(os.path.getsize(os.path.join(HERE, "e2e_sumgan_att.npz")) / 1024, "KB")
