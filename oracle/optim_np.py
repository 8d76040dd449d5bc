"""float64 restatement of the optimiser step the trainers take (reference: torch.optim.Adam(lr, weight_decay) at
summarizer/models/vasnet.py:181, dsn.py:70-73, behind torch.nn.utils.clip_grad_norm_ at dsn.py:145).  TEST INFRASTRUCTURE ONLY.

Plain numpy over one flat vector: the high-precision reference of tests/test_gpu_optim.py (csrc/optim.hip, training.FlatAdam),
pinned to stock torch.optim.Adam + clip_grad_norm_ run in float64 by tests/test_oracle.py.
"""
import numpy as np


def clip_coef(grad, grad_scale=1.0, max_norm=None):
    """clip_grad_norm_: coef = min(1, max_norm / (||grad_scale * grad||_2 + 1e-6)); 1 when no clip is asked for."""
    if max_norm is None:
        return 1.0
    g = np.asarray(grad, dtype=np.float64) * float(grad_scale)
    norm = float(np.sqrt(np.sum(g * g)))
    return min(1.0, float(max_norm) / (norm + 1e-6))


class AdamF64:
    """torch.optim.Adam (amsgrad=False, maximize=False) over a flat float64 vector, carrying m, v and the step count.
    step(grad, grad_scale, max_norm): the gradient is scaled, then clipped (norm of the SCALED gradient), then weight decay
    is added -- the order `loss / world -> clip_grad_norm_ -> optimizer.step()` produces."""

    def __init__(self, param, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, exp_avg=None, exp_avg_sq=None, step=0):
        self.p = np.array(param, dtype=np.float64).reshape(-1)
        self.m = np.zeros_like(self.p) if exp_avg is None else np.array(exp_avg, dtype=np.float64).reshape(-1)
        self.v = np.zeros_like(self.p) if exp_avg_sq is None else np.array(exp_avg_sq, dtype=np.float64).reshape(-1)
        self.lr, self.wd, self.betas, self.eps, self.t = float(lr), float(weight_decay), betas, float(eps), int(step)

    def step(self, grad, grad_scale=1.0, max_norm=None):
        """One step; returns the clip coefficient that was applied."""
        b1, b2 = float(self.betas[0]), float(self.betas[1])
        coef = clip_coef(grad, grad_scale, max_norm)
        g = np.asarray(grad, dtype=np.float64).reshape(-1) * float(grad_scale) * coef + self.wd * self.p
        self.t += 1
        self.m = b1 * self.m + (1.0 - b1) * g
        self.v = b2 * self.v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        self.p = self.p - (self.lr / bc1) * self.m / (np.sqrt(self.v) / np.sqrt(bc2) + self.eps)
        return coef
