"""Logistic-regression baseline on MI355X -- drop-in for `summarizer/models/logistic.py` (opt-in alias "logistic").

Same constructor (logistic.py:16), same attributes and state_dict keys (`perceptron.weight`, `perceptron.bias`) and the same
seeded initial weights (nn.Linear(input_size, 1) is created the same way), same forward contract x (seq_len, batch, input_size)
-> (seq_len, batch, 1) (logistic.py:23-36).  Scoring runs through the frame-head kernel (FrameHeadFunction: sigmoid(x w^T + b),
autograd included); the trainer's optimiser step is ONE kernel (sumk_logistic_step, csrc/logistic.hip).
"""
import random
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from .. import kernels
from .._lib import SumkError
from ..autograd import FrameHeadFunction
from . import Trainer
from ..training import FlatAdam, broadcast_parameters, dist_info, plan_shards, step_video_total


class LogisticRegression(nn.Module):
    def __init__(self, input_size=1024):
        super().__init__()
        self.input_size = input_size
        self.perceptron = nn.Linear(input_size, 1)
        self.sig = nn.Sigmoid()          # kept for the reference's attribute set; the kernel applies the sigmoid

    def _head(self, x):
        w, b = self.perceptron.weight, self.perceptron.bias
        for t, what in ((x, "logistic input"), (w, "perceptron.weight"), (b, "perceptron.bias")):
            kernels._require_gpu(t, what)
        return FrameHeadFunction.apply(x, w, b)

    def forward(self, x):
        """Each time step is predicted individually: x (seq_len, batch_size, input_size) -> scores (seq_len, batch_size, 1)."""
        seq_len, batch_size, input_size = x.shape
        assert self.input_size == input_size
        return self._head(x.reshape(-1, input_size)).view(seq_len, batch_size, 1)

    def score_packed(self, x_packed, lens):
        """Scores (n_rows,) of videos packed back to back (the trainers' batched scoring path): rows are independent here."""
        return self._head(x_packed)


def _batch_videos(extra_params):
    raw = str((extra_params or {}).get("batch_videos", 1))
    if raw == "auto":
        raise SumkError("LogisticRegressionTrainer: batch_videos='auto' is not supported (there is no step-cost model for this "
                        "model); give an integer number of videos per optimiser step (default 1, the reference's schedule)")
    bv = int(raw)
    if bv < 1:
        raise SumkError(f"LogisticRegressionTrainer: batch_videos must be >= 1, got {bv}")
    return bv


class LogisticRegressionTrainer(Trainer):
    """Mirror of the reference trainer (logistic.py:38-112): per-video nn.MSELoss to the min-max normalised gtscore,
    Adam(lr, weight_decay), periodic test, best-correlation weights.

    Each optimiser step is one sumk_logistic_step launch on a FlatAdam's buckets (forward, loss, backward and Adam in one kernel);
    the losses stay on the device and are read once per epoch.  Extensions (defaults = the reference schedule):
    extra_params["input_size"]; extra_params["batch_videos"] = videos per optimiser step (integer, default 1; the loss is then the
    mean over the step's videos of the per-video MSE); extra_params["hip_graph"] = "0" keeps every step eager -- otherwise, in a
    single process with one video per step, each video's step is captured once into a HIP graph and replayed from the second epoch
    on.  Under torch.distributed the videos are sharded over ranks (training.plan_shards), the kernel only accumulates the
    gradient, and FlatAdam all-reduces it and steps."""

    def _init_model(self):
        ep = self.hps.extra_params or {}
        model = LogisticRegression(**({"input_size": int(ep["input_size"])} if "input_size" in ep else {}))
        if self.hps.use_cuda:
            torch.cuda.set_device(self.hps.cuda_device)
            model.cuda()
        return model

    def train(self, fold):
        self.model.train()
        train_keys, _ = self._get_train_test_keys(fold)
        self.draw_gtscores(fold, train_keys)
        ep = self.hps.extra_params or {}
        dev = self._device()
        rank, world = dist_info()
        bv = _batch_videos(ep)
        broadcast_parameters(self.model)           # identical initial weights on every rank (one collective)
        self.optimizer = opt = FlatAdam(self.model.parameters(), lr=self.hps.lr, weight_decay=self.hps.weight_decay)
        frames = {k: int(self.dataset[k]["features"].shape[0]) for k in train_keys}
        my_keys, sizes, steps_per_epoch = plan_shards(train_keys, lambda: [frames[k] for k in train_keys], bv)
        # ONE workspace for the fold, sized for its largest step (captured steps hold its address)
        mine = sorted((frames[k] for k in my_keys), reverse=True)
        ws = torch.empty(max(1, kernels.logistic_step_workspace_bytes(max(1, sum(mine[:bv])), self.model.input_size)),
                         dtype=torch.uint8, device=dev)
        use_graph = (world == 1 and bv == 1 and dev.type == "cuda"
                     and str(ep.get("hip_graph", "1")) not in ("0", "False", "false"))
        graphs, pool = {}, None

        best = self._fold_best()
        for epoch in range(self.hps.epochs):
            losses, dist_scores = [], {}
            random.shuffle(my_keys)
            for step in range(steps_per_epoch):
                keys = my_keys[step * bv:(step + 1) * bv]
                if use_graph and epoch >= 1 and keys:
                    ent = graphs.get(keys[0])
                    if ent is None:
                        try:
                            ent = graphs[keys[0]] = self._capture_step(keys[0], dev, ws, pool)
                            if ent:
                                pool = ent.graph.pool()
                        except Exception as e:      # noqa: BLE001  (a configuration that does not capture keeps the eager loop)
                            self.log.warning(f"HIP graph capture failed ({type(e).__name__}: {e}); training continues eagerly")
                            use_graph, ent = False, False
                            torch.cuda.synchronize(dev)
                    if ent:
                        ent.graph.replay()
                        kernels.WEIGHTS_EPOCH[0] += 1
                        losses.append(ent.loss); dist_scores[keys[0]] = ent.scores
                        continue
                if world == 1:
                    loss, scores, lens = self._step(keys, dev, ws, 1.0 / len(keys), apply_adam=True)
                    opt.step_count += 1                   # (host mirror; the kernel advanced the device counter)
                else:
                    # data parallel: every video of the GLOBAL step weighs 1 / (videos of all ranks at this step)
                    opt.zero_grad()
                    if keys:
                        loss, scores, lens = self._step(keys, dev, ws, 1.0 / step_video_total(sizes, bv, step), apply_adam=False)
                    scale = opt.all_reduce_grads(average=False)
                    opt.step(grad_scale=scale)
                if keys:
                    losses.append(loss)
                    self._keep_scores(dist_scores, keys, scores, lens)

            # one D2H per epoch; the mean in float64 like the reference's np.mean over float(loss) values
            self._log_epoch(fold, epoch, Loss=float(np.mean(torch.cat(losses).cpu().numpy().astype(np.float64))) if losses else float("nan"))

            self._evaluate_epoch(fold, epoch, best)

        self.draw_scores(fold, dist_scores)
        return best[0], best[1], best[2]

    def _step(self, keys, dev, ws, scale, apply_adam):
        """One sumk_logistic_step over `keys` packed: (loss (1,), scores (n_rows,), lens)."""
        x, t, lens, sb = self._packed_batch(keys, dev)
        opt = self.optimizer
        loss, _, scores = kernels.logistic_step(x, sb, t, opt.flat_param, opt.flat_grad, opt.exp_avg,
                                                opt.exp_avg_sq, opt._state, opt.lr, opt.betas, opt.eps, opt.weight_decay, scale,
                                                apply_adam=apply_adam, want_scores=True, ws=ws)
        return loss, scores, lens

    def _capture_step(self, key, dev, ws, pool):
        """The step of `key` captured into a HIP graph (the memset node of the ticket block + the step kernel), with its static outputs;
        False when the video is not resident in the HBM cache (the graph records the addresses of its features and target)."""
        self._video_on_device(key, dev, want_target=True)
        video = self._hbm.get((key, str(dev)))
        if video is None:
            return False
        x, t = video
        sb = kernels.SeqBatch.get([x.shape[0]], dev)
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        mse = torch.zeros(1, dtype=torch.float32, device=dev)
        scores = torch.zeros(x.shape[0], dtype=torch.float32, device=dev)
        opt = self.optimizer
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=pool):
            kernels.logistic_step(x, sb, t, opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq, opt._state, opt.lr, opt.betas,
                                  opt.eps, opt.weight_decay, 1.0, apply_adam=True, loss=loss, mse=mse, scores=scores, ws=ws)
        return SimpleNamespace(graph=g, loss=loss, scores=scores.view(-1, 1, 1), keep=(sb, video, mse))
