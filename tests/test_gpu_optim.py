"""GPU: the optimiser step every trainer ends in (csrc/optim.hip: adam_prep_kernel + adam_kernel<ZERO>, sumsq, the bf16 casts; training.FlatAdam)
against the float64 restatement oracle/optim_np.AdamF64 (pinned to torch.optim.Adam + clip_grad_norm_ in float64 by tests/test_oracle.py).

Gates come from arithmetic, as in tests/test_gpu_transformer_f64.py: stock torch.optim.Adam (+ torch.nn.utils.clip_grad_norm_) run in fp32
on the CPU on the same inputs is the yardstick, its distance to the float64 reference; each HIP buffer must stay within 4 x the yardstick,
and the yardstick has a floor of 2 fp32 ulps of the value (a buffer of one or three elements can land on the float64 value by chance).
The factor 4 covers a different but legitimate operation order (sqrt(v) * inv_sqrt_bc2 here, a division in torch; fp32 scale constants
rounded from double here).  The error of a buffer is its largest element-wise relative error (_relerr); no element is left out.  Elements
whose sqrt(v_hat) is within a factor 10 of eps would amplify rounding: gradients are drawn with |g| >= 0.05 x their spread (_grad; the
issue asks for at least 1e-3) and every case asserts on the
float64 reference that it has none.  sumsq: 4 x the error of torch.sum(x * x) in fp32, floor 4 ulps.

The worst ratio (HIP error / yardstick) of every case is printed and kept in REPORT (written to $SUMK_REPORT_DIR when set)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import optim_np

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -24
GRID = 4 * 256 * 2048                       # elements one grid pass of adam_kernel / the cast kernels covers (2048 blocks x 256 lanes x float4)
VASNET_BUCKET = 5246977                     # trainable parameters of VASNet(D = 1024); FlatAdam pads the bucket to 5246980
LR, EPS, BETAS = 5e-3, 1e-8, (0.9, 0.999)
REPORT = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for r in REPORT:
        print("OPTIM-REPORT", json.dumps(r))
    d = os.environ.get("SUMK_REPORT_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "optim_f64.json"), "w") as f:
            json.dump(REPORT, f, indent=1)


# ------------------------------------------------------------------------------------------------ inputs
def _grad(rng, n, scale=1.0, floor=0.05):
    """Signed gradients with |g| >= floor * scale.  The floor keeps every scaled, clipped gradient of this file far above both 1e-3 x its
    own spread and weight_decay x |param| (at most 1e-5 x 5, or 1e-2 x 0.6 in the pad-lane case), so g + wd p never cancels to ~eps."""
    g = rng.standard_normal(n)
    return ((np.sign(g) + (g == 0)) * (floor + np.abs(g)) * scale).astype(np.float32)


def _with_scaled_norm(g, target, grad_scale):
    """g (float32) rescaled so that the float64 norm of grad_scale * g is `target` (to fp32 rounding of the elements)."""
    for _ in range(3):
        norm = float(np.sqrt(np.sum((g.astype(np.float64) * grad_scale) ** 2)))
        g = (g.astype(np.float64) * (target / norm)).astype(np.float32)
    return g


def _relerr(got, ref):
    """Largest element-wise error relative to max(|reference element|, RMS of the reference buffer); where the reference is exactly 0 the
    value must be exactly 0.  Every element is a sum of terms of about the buffer's RMS size (param - update, b1 m + (1 - b1) g), so an
    element that lands near 0 carries the rounding of those terms: measured against its own tiny value, its relative error is a
    heavy-tailed cancellation figure (1e-4 and more for a parameter of 1e-5, in torch's fp32 run and in the kernel's alike, on different
    elements), and the maximum over a buffer compares two outliers instead of two implementations."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    zero = ref == 0
    assert (got[zero] == 0).all()
    if zero.all():
        return 0.0
    rms = float(np.sqrt(np.mean(ref[~zero] ** 2)))
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.maximum(np.abs(ref[~zero]), rms)))


class Torch32:
    """The yardstick: stock torch.optim.Adam + clip_grad_norm_ in fp32 on the CPU, optionally resumed from given moments and step count."""

    def __init__(self, p0, lr, wd, m0=None, v0=None, step=0):
        self.p = torch.nn.Parameter(torch.from_numpy(np.array(p0, np.float32)))
        self.opt = torch.optim.Adam([self.p], lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
        if step:
            self.opt.state[self.p] = dict(step=torch.tensor(float(step)), exp_avg=torch.from_numpy(np.array(m0, np.float32)),
                                          exp_avg_sq=torch.from_numpy(np.array(v0, np.float32)))
        self.gs_eff = None

    def step(self, g, grad_scale, max_norm):
        self.p.grad = torch.from_numpy(np.array(g, np.float32)) * np.float32(grad_scale)
        coef = 1.0
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_([self.p], max_norm)
            coef = float(torch.clamp(max_norm / (tn + 1e-6), max=1.0))
        self.gs_eff = float(np.float32(grad_scale) * np.float32(coef))
        self.opt.step()

    def buffers(self):
        st = self.opt.state[self.p]
        return self.p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


class HipBuffers:
    """The raw kernel entries on four flat device buffers + the device state block."""

    def __init__(self, dev, entry, p0, lr, wd, m0=None, v0=None, step=0):
        self.entry, self.lr, self.wd, self.t = entry, lr, wd, step
        f = lambda a: torch.from_numpy(np.array(a, np.float32)).to(dev)
        self.p, self.m, self.v = f(p0), f(np.zeros_like(p0) if m0 is None else m0), f(np.zeros_like(p0) if v0 is None else v0)
        self.g = torch.zeros_like(self.p)
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)
        self.state[0] = step
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)

    def step(self, g, grad_scale, max_norm):
        from summarizer_amd import kernels
        self.g.copy_(torch.from_numpy(g))
        self.t += 1
        if self.entry == "adam_step":
            assert max_norm is None
            kernels.adam_step(self.p, self.g, self.m, self.v, self.t, self.lr, BETAS, EPS, self.wd, grad_scale)
            return
        sumsq = None
        if max_norm is not None:
            self.norm.zero_()
            sumsq = kernels.sumsq(self.g, out=self.norm)
        kernels.adam_step_dev(self.p, self.g, self.m, self.v, self.state, self.lr, BETAS, EPS, self.wd, grad_scale, sumsq,
                              0.0 if max_norm is None else max_norm, zero_grad=self.entry == "dev_zero")

    def buffers(self):
        return self.p.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy()

    def grad(self):
        return self.g.cpu().numpy()

    def dev_state(self):
        return self.state.cpu() if self.entry != "adam_step" else None

    zeroes = property(lambda self: self.entry == "dev_zero")


class HipFlat:
    """training.FlatAdam.step on a real module."""

    def __init__(self, opt, zero_grad):
        self.opt, self.zero, self.entry = opt, zero_grad, "FlatAdam"

    def step(self, g, grad_scale, max_norm):
        self.opt.flat_grad[:g.shape[0]].copy_(torch.from_numpy(g))
        self.opt.step(grad_scale=grad_scale, max_norm=max_norm, zero_grad=self.zero)

    def buffers(self):
        n = self.opt.n
        return self.opt.flat_param[:n].cpu().numpy(), self.opt.exp_avg[:n].cpu().numpy(), self.opt.exp_avg_sq[:n].cpu().numpy()

    def grad(self):
        return self.opt.flat_grad[:self.opt.n].cpu().numpy()

    def dev_state(self):
        return self.opt._state.cpu()

    zeroes = property(lambda self: self.zero)


def _run(cid, hip, p0, grads, lr, wd, grad_scale, max_norm, m0=None, v0=None, step0=0, expect_coef=None):
    """Step the float64 reference, the fp32 torch yardstick and the HIP entry through `grads`; after every step compare param, exp_avg,
    exp_avg_sq, the gradient buffer and the device state.  expect_coef: predicate on the reference's clip coefficient (the case's side)."""
    ref = optim_np.AdamF64(p0, lr, wd, BETAS, EPS, exp_avg=m0, exp_avg_sq=v0, step=step0)
    t32 = Torch32(p0, lr, wd, m0, v0, step0)
    worst = {}
    for g in grads:
        coef = ref.step(g, grad_scale, max_norm)
        if expect_coef is not None:
            assert expect_coef(coef), (cid, coef)
        t32.step(g, grad_scale, max_norm)
        hip.step(g, grad_scale, max_norm)
        bc2 = 1.0 - BETAS[1] ** ref.t
        assert np.sqrt(ref.v / bc2).min() > 10 * EPS, (cid, "an element's sqrt(v_hat) is within a factor 10 of eps")
        for name, got, r64, r32 in zip(("param", "exp_avg", "exp_avg_sq"), hip.buffers(), (ref.p, ref.m, ref.v), t32.buffers()):
            assert np.isfinite(got).all(), (cid, name)
            yard = max(_relerr(r32, r64), 2 * ULP)
            err = _relerr(got, r64)
            worst[name] = max(worst.get(name, 0.0), err / yard)
            assert err <= 4 * yard, (cid, hip.entry, name, "step", ref.t, err, yard)
        gb = hip.grad()
        if hip.zeroes:
            assert not gb.any(), (cid, "gradient buffer not zero after zero_grad=True")
        else:
            assert np.array_equal(gb.view(np.uint32), np.asarray(g).view(np.uint32)), (cid, "gradient buffer changed")
        st = hip.dev_state()
        if st is not None:
            assert int(st[0]) == ref.t, (cid, int(st[0]), ref.t)
            f = st.view(torch.float32).numpy().astype(np.float64)
            # state[1..3]: step size, 1 / sqrt(bias correction 2) and the effective gradient scale, computed in double from fp32 arguments
            # and rounded once (2 ulps); the clip coefficient carries the fp32 sum of squares: torch's own fp32 coefficient is its yardstick
            assert abs(f[1] - lr / (1 - BETAS[0] ** ref.t)) <= 2 * ULP * f[1] and abs(f[2] - 1 / np.sqrt(bc2)) <= 2 * ULP * f[2], (cid, f)
            want = grad_scale * coef
            yard = max(abs(t32.gs_eff - want) / want, 2 * ULP)
            worst["grad_scale_eff"] = max(worst.get("grad_scale_eff", 0.0), abs(f[3] - want) / want / yard)
            assert abs(f[3] - want) / want <= 4 * yard, (cid, "effective gradient scale", f[3], want, t32.gs_eff)
    REPORT.append(dict(case=cid, entry=hip.entry, n=int(np.asarray(p0).size), steps=len(grads), worst_ratio=worst))
    print("OPTIM", cid, hip.entry, {k: round(v, 3) for k, v in worst.items()})
    return ref


# ------------------------------------------------------------------------------------------------ sizes x entries
@pytest.mark.parametrize("entry", ["adam_step", "dev", "dev_zero"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 100003, GRID, GRID + 4, GRID + 7])
def test_adam_sizes_vs_float64(dev, entry, n):
    """float4 body, scalar tail (n not a multiple of 4), the grid-stride loop's second pass (GRID + 4: its first float4; GRID + 7: a tail
    behind it), two steps with weight decay and grad_scale 1/2."""
    rng = np.random.default_rng(1000 + n % 9973)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [_grad(rng, n) for _ in range(2)]
    _run(f"sizes_n{n}", HipBuffers(dev, entry, p0, LR, 1e-5), p0, grads, LR, 1e-5, 0.5, None)


# ------------------------------------------------------------------------------------------------ clip
MAX_NORM = 5.0
CLIP_CASES = {
    # id: (norm of the SCALED gradient, grad_scale, predicate on the float64 coefficient)
    "a_bites_0.1": (50.0, 1.0, lambda c: abs(c - 0.1) < 1e-6),
    "b_min_decides": (2.5, 1.0, lambda c: c == 1.0),                              # max_norm / norm = 2: without the min the gradient doubles
    "c_ulps_below_1": (MAX_NORM / (1 - 4 * ULP) - 1e-6, 1.0, lambda c: 1 - 16 * ULP < c < 1.0),
    "c_ulps_above_1": (MAX_NORM / (1 + 4 * ULP) - 1e-6, 1.0, lambda c: c == 1.0),   # (raw coefficient a few ulps above 1: asserted in the test)
    "d_scale_eighth_idle": (2.5, 0.125, lambda c: c == 1.0),                      # unscaled norm 20: a norm without grad_scale would clip to 0.25
    "d_scale_half_bites": (8.0, 0.5, lambda c: abs(c - 0.625) < 1e-6),            # unscaled norm 16: a norm without grad_scale gives 0.3125
}


@pytest.mark.parametrize("entry", ["dev", "dev_zero"])
@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_adam_clip_coefficient_vs_float64(dev, entry, case):
    norm, gs, pred = CLIP_CASES[case]
    n = 100004
    rng = np.random.default_rng(sorted(CLIP_CASES).index(case) + 50)
    p0 = rng.standard_normal(n).astype(np.float32)
    g = _with_scaled_norm(_grad(rng, n), norm, gs)
    assert np.abs(g).min() * gs * min(1.0, MAX_NORM / norm) > 1e-4
    raw = MAX_NORM / (float(np.sqrt(np.sum((g.astype(np.float64) * gs) ** 2))) + 1e-6)
    if case.startswith("c_"):                                                    # within a few ulps of 1, on the side the name says
        assert abs(raw - 1) < 16 * ULP and (raw > 1) == case.endswith("above_1") and raw != 1, (case, raw)
    _run(f"clip_{case}", HipBuffers(dev, entry, p0, LR, 1e-5), p0, [g], LR, 1e-5, gs, MAX_NORM, expect_coef=pred)


@pytest.mark.parametrize("entry", ["dev", "dev_zero"])
def test_adam_clip_of_an_all_zero_gradient(dev, entry):
    """0 / (0 + 1e-6): coefficient 1 and no NaN.  The zero gradient is the second step, so the moments are not zero (sqrt(v_hat) >> eps)."""
    n = 1028
    rng = np.random.default_rng(61)
    p0 = rng.standard_normal(n).astype(np.float32)
    _run("clip_e_zero_gradient", HipBuffers(dev, entry, p0, LR, 0.0), p0, [_grad(rng, n), np.zeros(n, np.float32)], LR, 0.0, 0.125, MAX_NORM,
         expect_coef=lambda c: 0 < c <= 1.0)
    ref = optim_np.AdamF64(p0, LR)
    assert ref.step(np.zeros(n), 0.125, MAX_NORM) == 1.0


# ------------------------------------------------------------------------------------------------ steps
@pytest.mark.parametrize("entry", ["adam_step", "dev", "dev_zero"])
def test_adam_ten_steps_vs_float64(dev, entry):
    n = 100003
    rng = np.random.default_rng(70)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [_grad(rng, n, scale=0.05 * (1 + k)) for k in range(10)]              # norms 16 .. 160 before grad_scale 1/8: the clip bites from step 3 on
    clip = None if entry == "adam_step" else MAX_NORM
    _run("ten_steps", HipBuffers(dev, entry, p0, LR, 1e-5), p0, grads, LR, 1e-5, 0.125, clip)


@pytest.mark.parametrize("entry", ["adam_step", "dev", "dev_zero"])
@pytest.mark.parametrize("step0", [9999, 1000000])
def test_adam_bias_correction_at_a_large_step_count(dev, entry, step0):
    """state[0] preset: 1 - 0.999^10000 = 0.99995, 1 - 0.999^1000001 = 1 to double precision (pow in double on the device); the moments
    come from three float64 reference steps, rounded to fp32 so that all three implementations resume from the same numbers."""
    n = 4100
    rng = np.random.default_rng(80 + step0 % 7)
    p0 = rng.standard_normal(n).astype(np.float32)
    seed = optim_np.AdamF64(p0, LR, 1e-5, BETAS, EPS)
    for _ in range(3):
        seed.step(_grad(rng, n))
    p1, m1, v1 = seed.p.astype(np.float32), seed.m.astype(np.float32), seed.v.astype(np.float32)
    hip = HipBuffers(dev, entry, p1, LR, 1e-5, m1, v1, step=step0)
    ref = _run(f"step0_{step0}", hip, p1, [_grad(rng, n)], LR, 1e-5, 1.0, None if entry == "adam_step" else MAX_NORM, m1, v1, step0)
    assert ref.t == step0 + 1


# ------------------------------------------------------------------------------------------------ zero_grad folded into the step
@pytest.mark.parametrize("n", [5, 1023, GRID + 7])
def test_zero_grad_step_gives_the_same_bits(dev, n):
    rng = np.random.default_rng(90)
    p0 = rng.standard_normal(n).astype(np.float32)
    a, b = HipBuffers(dev, "dev", p0, LR, 1e-5), HipBuffers(dev, "dev_zero", p0, LR, 1e-5)
    for k in range(3):
        g = _grad(rng, n, scale=3.0)
        a.step(g, 0.5, MAX_NORM); b.step(g, 0.5, MAX_NORM)
        for x, y in zip(a.buffers(), b.buffers()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert torch.equal(a.state, b.state)
        assert not b.grad().any() and np.array_equal(a.grad(), g)


# ------------------------------------------------------------------------------------------------ FlatAdam on real modules
def _vasnet(dev):
    from summarizer_amd.models.vasnet import VASNet
    torch.manual_seed(3)
    return VASNet(input_size=1024).to(dev)


@pytest.mark.parametrize("zero_grad", [False, True])
def test_flat_adam_on_the_vasnet_bucket_vs_float64(dev, zero_grad):
    """The ~5.2 M-element bucket of VASNet(D = 1024): two and a half grid passes of adam_kernel, the stride loop of sumsq; clip biting with
    grad_scale 1/2; three steps.  The three pad lanes stay exactly 0 in all four buffers."""
    from summarizer_amd.training import FlatAdam
    model = _vasnet(dev)
    opt = FlatAdam(model.parameters(), LR, weight_decay=1e-5)
    n = opt.n
    assert n == VASNET_BUCKET and opt.flat_param.numel() == n + 3 and n > 2 * GRID
    p0 = opt.flat_param[:n].cpu().numpy()
    rng = np.random.default_rng(100)
    grads = [_grad(rng, n, scale=0.01) for _ in range(3)]                         # norm ~ 0.01 x 0.8 x sqrt(5.2e6) = 18, scaled 9 > 5
    _run("vasnet_bucket", HipFlat(opt, zero_grad), p0, grads, LR, 1e-5, 0.5, MAX_NORM, expect_coef=lambda c: 0.3 < c < 0.9)
    for buf in (opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq):
        assert not buf[n:].cpu().numpy().view(np.uint32).any()
    assert model.K.weight.data_ptr() >= opt.flat_param.data_ptr() and opt.step_count == 3


def _small_module(dev):
    torch.manual_seed(5)
    return torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Tanh(), torch.nn.Linear(3, 1, bias=False)).to(dev)      # 15 + 3 + 3 = 21 -> 3 pad lanes


@pytest.mark.parametrize("zero_grad", [False, True])
def test_flat_adam_pad_lanes_stay_zero(dev, zero_grad):
    from summarizer_amd.training import FlatAdam
    mod = _small_module(dev)
    opt = FlatAdam(mod.parameters(), LR, weight_decay=1e-2)
    n = opt.n
    assert n == 21 and opt.flat_param.numel() == 24
    p0 = opt.flat_param[:n].cpu().numpy()
    rng = np.random.default_rng(110)
    _run("pad_lanes", HipFlat(opt, zero_grad), p0, [_grad(rng, n, scale=2.0) for _ in range(10)], LR, 1e-2, 0.5, MAX_NORM)
    for buf in (opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq):
        assert not buf[n:].cpu().numpy().view(np.uint32).any()
    # the parameters are views of the bucket: the module computes with the stepped weights
    assert torch.equal(mod[0].weight.reshape(-1), opt.flat_param[:15])


def test_zeroed_by_step_then_accumulated_backward_equals_plain_zero_grad(dev):
    """step(zero_grad=True) -> zero_grad(zeroed_by_step=True) (no fill launch) -> two backward passes accumulating into the bucket gives
    the bits of step(zero_grad=False) -> zero_grad() -> the same two passes."""
    from summarizer_amd.training import FlatAdam
    x = torch.from_numpy(np.random.default_rng(120).standard_normal((2, 7, 5)).astype(np.float32)).to(dev)
    out = []
    for folded in (False, True):
        mod = _small_module(dev)
        opt = FlatAdam(mod.parameters(), LR, weight_decay=1e-5)
        for k in range(2):
            opt.zero_grad(zeroed_by_step=folded)
            for xb in x:
                mod(xb).square().mean().backward()
            assert opt.flat_grad[:opt.n].abs().min() > 0
            opt.step(grad_scale=0.5, max_norm=MAX_NORM, zero_grad=folded)
            assert bool(opt.flat_grad.any()) != folded
        opt.zero_grad(zeroed_by_step=folded)
        assert not opt.flat_grad.any()
        for xb in x:
            mod(xb).square().mean().backward()
        out.append([t.clone() for t in (opt.flat_grad, opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt._state[:1])])
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not out[0][0][21:].any() and out[0][0][:21].abs().min() > 0


# ------------------------------------------------------------------------------------------------ sumsq
def _sumsq_input(n, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "spiky":                                                          # a few entries 1e4 times larger than the rest
        x[rng.choice(n, size=min(n, 5), replace=False)] *= np.float32(1e4)
    return x


@pytest.mark.parametrize("kind", ["normal", "spiky"])
@pytest.mark.parametrize("n", [1, 63, 64, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1, VASNET_BUCKET + 3])
def test_sumsq_vs_float64(dev, n, kind):
    """One block, a partly filled wave, the 1024-block cap (1024 x 1024 + 1 is the first size whose blocks stride), the VASNet bucket; the
    documented `out[0] += sum`; the same bits on a second run and after the cached workspace was filled with 0xFF bytes."""
    from summarizer_amd import kernels
    x = _sumsq_input(n, kind, 130 + n % 1000)
    xd = torch.from_numpy(x).to(dev)
    ref = float(np.sum(x.astype(np.float64) ** 2))
    xc = torch.from_numpy(x)
    yard = max(abs(float(torch.sum(xc * xc)) - ref), 4 * ULP * ref)              # torch.sum(x * x) in fp32 (CPU, like the Adam yardstick)
    s1 = kernels.sumsq(xd)
    err = abs(float(s1) - ref)
    REPORT.append(dict(case=f"sumsq_{kind}_n{n}", worst_ratio=err / yard, rel_err=err / ref))
    print("OPTIM sumsq", kind, n, "err/yard", round(err / yard, 3), "rel", err / ref)
    assert err <= 4 * yard, (n, kind, float(s1), ref, yard)
    assert torch.equal(kernels.sumsq(xd), s1)                                    # deterministic
    kernels._sumsq_ws[str(xd.device)].fill_(255)
    assert torch.equal(kernels.sumsq(xd), s1)                                    # the workspace is written before it is read
    # accumulate-into-out: a second vector's sum is ADDED to what `out` holds (one fp32 addition of the two sums)
    y = torch.from_numpy(_sumsq_input(n, "normal", 7 + n % 1000)).to(dev)
    s2 = kernels.sumsq(y)
    acc = s1.clone()
    assert kernels.sumsq(y, out=acc) is acc
    assert float(s2) > 0 and torch.equal(acc, s1 + s2)


# ------------------------------------------------------------------------------------------------ casts
SPECIAL_BITS = np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,      # +-0, +-inf, quiet / signalling NaNs
    0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80008000, 0x00010000,      # subnormals (0x00008000: tie to 0; 0x00018000: tie up to 0x0002)
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                                          # exact ties: down to even 0x3F80, up to even 0x3F82
    0x3F808001, 0x3F807FFF, 0x3F80FFFF,                                                      # one ulp either side of a tie; carries into the next bf16
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,                                          # largest finite -> inf; the tie below inf (-> inf); largest that stays finite
    0x3F800000, 0x477FE000, 0x00800000,
], dtype=np.uint32)


def _cast_input(n, seed):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    k = min(n, len(SPECIAL_BITS))
    bits[:k] = SPECIAL_BITS[:k]
    if n > 2 * len(SPECIAL_BITS):
        bits[-len(SPECIAL_BITS):] = SPECIAL_BITS[::-1]                          # the scalar tail and the last float4 see them too
    return bits


@pytest.mark.parametrize("n", [1, 3, 4, 5, 100003, GRID + 5])
def test_cast_f32_bf16_bit_equal_to_torch(dev, n):
    from summarizer_amd import kernels
    for rep in range(len(SPECIAL_BITS) if n <= 5 else 1):                         # (the small sizes: every special value passes through them)
        bits = _cast_input(n, 140 + n % 1000)
        if n <= 5:
            bits[:] = np.roll(SPECIAL_BITS, -rep)[:n]
        src = torch.from_numpy(bits.view(np.float32).copy())
        want = src.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        dst = torch.full((n,), -1, dtype=torch.int16, device=dev).view(torch.bfloat16)
        kernels.cast_f32_bf16(src.to(dev), dst)
        got = dst.view(torch.int16).cpu().numpy().view(np.uint16)
        nan = np.isnan(bits.view(np.float32))
        assert ((want[nan] & 0x7F80) == 0x7F80).all() and ((want[nan] & 0x7F) != 0).all()
        assert ((got[nan] & 0x7F80) == 0x7F80).all() and ((got[nan] & 0x7F) != 0).all(), "a NaN did not stay a NaN"
        bad = np.flatnonzero(got[~nan] != want[~nan])
        assert bad.size == 0, (n, [hex(b) for b in bits[~nan][bad][:8]], [hex(b) for b in got[~nan][bad][:8]], [hex(b) for b in want[~nan][bad][:8]])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 100003, GRID + 5])
def test_cast_bf16_f32_bit_equal_to_torch(dev, n):
    """Every one of the 65 536 bf16 bit patterns (the large sizes hold them all, head and tail)."""
    from summarizer_amd import kernels
    every = np.arange(65536, dtype=np.uint16)
    for rep in range(16 if n <= 5 else 1):
        bits = np.resize(every, n).copy()
        if n <= 5:
            bits[:] = (SPECIAL_BITS >> 16).astype(np.uint16)[rep:rep + n]
        else:
            assert np.unique(bits).size == 65536
            bits[-4:] = np.array([0x7F80, 0xFFC1, 0x0001, 0x8000], dtype=np.uint16)
        src = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
        want = src.float().numpy().view(np.uint32)
        dst = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        kernels.cast_bf16_f32(src.to(dev), dst)
        got = dst.cpu().numpy().view(np.uint32)
        nan = np.isnan(want.view(np.float32))
        assert np.isnan(got.view(np.float32)[nan]).all()
        assert np.array_equal(got[~nan], want[~nan])
        assert np.array_equal(want[~nan], bits[~nan].astype(np.uint32) << 16)     # (the conversion is a shift: the reference itself, restated)
