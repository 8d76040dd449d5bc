"""Random-scores baseline -- drop-in for `summarizer/models/rand.py` (opt-in alias "random").

The scores are drawn from torch's CPU generator and then moved to the input's device, exactly as rand.py:27-28 does, so under the
same seed they are bit-identical to the reference's.  The trainer's logged losses come from the per-video MSE kernel
(sumk_segment_mse_forward, one launch per epoch for all training videos) and its test takes the base Trainer's device evaluation tail.
"""
import random

import numpy as np
import torch
import torch.nn as nn

from .. import kernels
from ..autograd import SegmentMseFunction
from . import Trainer


class Random(nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, x):
        """x (seq_len, batch_size, input_size) -> probs (seq_len, batch_size, 1), uniform in [0, 1)."""
        seq_len, batch_size, _ = x.shape
        scores = torch.rand((seq_len, batch_size, 1))
        return scores.to(x.device)

    def score_packed(self, x_packed, lens):
        """Scores (n_rows,) of videos packed back to back.  One draw of shape (T, 1, 1) per video, in order: the generator stream of
        the reference's per-video test loop (models/__init__.py:42-49 of the reference), then ONE host-to-device copy."""
        draws = [torch.rand((int(T), 1, 1)) for T in lens]
        return torch.cat(draws).view(-1).to(x_packed.device)


class RandomTrainer(Trainer):
    """Mirror of the reference trainer (rand.py:31-96): no optimisation; per epoch the training videos are scored (shuffled order),
    their MSE to the min-max normalised gtscore is logged, and the periodic test keeps the best-correlation "weights" (the empty
    state_dict)."""

    def _init_model(self):
        return Random()

    def train(self, fold):
        self.model.train()
        train_keys, _ = self._get_train_test_keys(fold)
        self.draw_gtscores(fold, train_keys)
        dev = self._device()

        best = self._fold_best()
        for epoch in range(self.hps.epochs):
            dist_scores = {}
            random.shuffle(train_keys)
            vids = [self._video_on_device(k, dev, want_target=True) for k in train_keys]
            scores = [self.model(v[0].unsqueeze(1)) for v in vids]        # one draw per video, in the shuffled order
            for k, s in zip(train_keys, scores):
                dist_scores[k] = s
            if train_keys:
                lens = [v[0].shape[0] for v in vids]
                mse = SegmentMseFunction.apply(torch.cat([s.view(-1) for s in scores]), torch.cat([v[1] for v in vids]),
                                               kernels.SeqBatch.get(lens, dev))
                # one D2H per epoch; the mean in float64 like the reference's np.mean over float(loss) values
                train_avg_loss = float(np.mean(mse.cpu().numpy().astype(np.float64)))
            else:
                train_avg_loss = float("nan")
            self._log_epoch(fold, epoch, Loss=train_avg_loss)

            self._evaluate_epoch(fold, epoch, best)

        self.draw_scores(fold, dist_scores)
        return best[0], best[1], best[2]
