"""Positional models (`max_pos`) on the packed path against the per-video route they took before, on the 50-video S-TVSum-shaped set
(12 003 frames at seed 11, D = 1024, max_pos = 320 = the longest video):
  * Trainer.test, VASNet fp32 and bf16x3: packed scoring + device tail  vs  one `forward` per video + the native host tail;
  * the single-video VASNet training step: the replayed HIP graph of the packed step  vs  the eager step through `forward`;
  * Transformer bf16x3 scoring (6 layers, 8 heads): one packed launch  vs  one `forward` per video.
The per-video routes are spelled out here the way the trainers ran them before, so one process times both.  Alternating rounds; medians
and every round's figure go to the JSON file named by the second argument (the record under profiles/ is such a file).
    python scripts/pos_packed_timing.py time OUT.json
    rocprofv3 --kernel-trace --stats ... -- python scripts/pos_packed_timing.py trace      (the positional kernels alone, beside add + split_planes)"""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summarizer_amd import kernels
from summarizer_amd.models.transformer import TransformerTrainer
from summarizer_amd.models.vasnet import VASNetTrainer
from summarizer_amd.training import FlatAdam
from summarizer_amd.utils.datasets import synthetic_dataset
from summarizer_amd.utils.hps import make_hps

mode = sys.argv[1] if len(sys.argv) > 1 else "time"
dev = torch.device("cuda:0")
ds = synthetic_dataset(50, seed=11, D=1024, t_range=(150, 320), n_users=20)
keys = list(ds.keys())
MAX_POS = 320


def trainer(cls, **extra):
    hps = make_hps(ds, [{"train_keys": keys, "test_keys": keys}], epochs=1, extra_params={"max_pos": str(MAX_POS), **extra})
    torch.manual_seed(1234)
    return cls(hps, hps.splits_files[0]).reset()


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, res


def per_video_test(tr):
    """Trainer.test as it ran for a positional model before: one forward per video (on a clone: the add is in place), host tail."""
    tr.model.eval()
    with torch.no_grad():
        acts = {k: tr.model(tr._video_on_device(k, dev)[0].unsqueeze(1).clone()).squeeze().detach().cpu().numpy() for k in keys}
    corr, f_avg, f_max, _ = tr._evaluate_native(acts, keys)
    return np.mean(corr), (np.mean(f_avg), np.mean(f_max))


if mode == "trace":
    lens = [int(ds[k]["features"].shape[0]) for k in keys]
    sb = kernels.SeqBatch.get(lens, dev)
    x = torch.randn(sum(lens), 1024, device=dev); table = torch.randn(MAX_POS, 1024, device=dev)
    pos = torch.cat([torch.arange(T) for T in lens]).to(dev)
    for _ in range(12):
        kernels.pos_add_packed(x, sb, table, want_f32=True)                              # fp32 alone
        kernels.pos_add_packed(x, sb, table, want_f32=True, want_bf16=True)              # fp32 + bf16 (the mixed-precision step)
        for npl in (2, 3):
            kernels.pos_add_packed(x, sb, table, want_f32=True, n_planes=npl)            # fused: fp32 + planes
            kernels.split_planes(kernels.pos_add_packed(x, sb, table, want_f32=True)[0], npl)      # fp32 add, then split_planes
        g = torch.zeros_like(table)
        kernels.pos_table_grad(x, sb, g)                                                 # the deterministic gather
        g.zero_().index_add_(0, pos, x)                                                  # torch's atomic scatter
    torch.cuda.synchronize()
    sys.exit(0)

out = {}
# ---- Trainer.test, VASNet fp32 / bf16x3
for prec in ("fp32", "bf16x3"):
    tr = trainer(VASNetTrainer, precision=prec)
    timed(lambda: tr.test(0), 5); timed(lambda: per_video_test(tr), 2)
    a, b = [], []
    for r in range(5):
        t, res_p = timed(lambda: tr.test(0), 30); a.append(t)
        t, res_v = timed(lambda: per_video_test(tr), 3); b.append(t)
    out[f"trainer_test_{prec}_packed_ms"], out[f"trainer_test_{prec}_per_video_ms"] = a, b
    out[f"trainer_test_{prec}_results"] = dict(packed=[float(res_p[0]), float(res_p[1][0]), float(res_p[1][1])],
                                               per_video=[float(res_v[0]), float(res_v[1][0]), float(res_v[1][1])])

# ---- the single-video training step: replayed graph of the packed step vs the eager per-video step through forward
tr = trainer(VASNetTrainer)
tr.model.train()
tr.optimizer = FlatAdam(tr.model.parameters(), lr=1e-5)
tr.model.graph_seed = torch.zeros(1, dtype=torch.int64, device=dev)
key = keys[0]
seq, target = tr._video_on_device(key, dev, want_target=True)
for _ in range(3):
    tr._single_video_step(key, dev)
graph = tr._capture_step(key, dev, None)


def eager_forward_step():
    tr.optimizer.zero_grad(zeroed_by_step=True)
    sc = tr.model(seq.unsqueeze(1).clone())
    loss = torch.mean((sc.view(-1) - target) ** 2)
    loss.backward(gradient=kernels.one(dev))
    tr.optimizer.step(grad_scale=1.0, zero_grad=True)


tr.model.graph_seed = None
timed(eager_forward_step, 10)
a, b, c = [], [], []
for r in range(5):
    tr.model.graph_seed = torch.zeros(1, dtype=torch.int64, device=dev)
    a.append(timed(graph[0].replay, 200)[0])
    c.append(timed(lambda: tr._single_video_step(key, dev), 50)[0])
    tr.model.graph_seed = None
    b.append(timed(eager_forward_step, 50)[0])
out["train_step_replayed_ms"], out["train_step_eager_packed_ms"], out["train_step_per_video_forward_ms"] = a, c, b
out["train_step_frames"] = int(seq.shape[0])

# ---- Transformer bf16x3 scoring
tr = trainer(TransformerTrainer, precision="bf16x3")
tr.model.eval()
feats = [tr._video_on_device(k, dev)[0] for k in keys]
lens = [f.shape[0] for f in feats]
packed = torch.cat(feats)


def tf_per_video():
    with torch.no_grad():
        return [tr.model(f.unsqueeze(1).clone()) for f in feats]


def tf_packed():
    with torch.no_grad():
        return tr.model.score_packed(packed, lens)


timed(tf_packed, 3); timed(tf_per_video, 1)
a, b = [], []
for r in range(5):
    a.append(timed(tf_packed, 10)[0]); b.append(timed(tf_per_video, 2)[0])
out["transformer_bf16x3_packed_ms"], out["transformer_bf16x3_per_video_ms"] = a, b
out["frames"] = int(sum(lens))
out["median"] = {k: float(np.median(v)) for k, v in out.items() if k.endswith("_ms")}
dest = sys.argv[2] if len(sys.argv) > 2 else "pos_packed_timing.json"
json.dump(out, open(dest, "w"), indent=1)
print(json.dumps(out["median"]))
