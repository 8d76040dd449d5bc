"""The input families of tests/test_gpu_attn_strip.py (csrc/attn_b16.hip through sumk_attn_strips_b16), built on the host so that
tests/test_attn_strip_host.py can run the float32 specification and its mutants through the same gates without a GPU.  TEST INFRASTRUCTURE ONLY.

A case is a dict: name, lens, D, scale, ignore_self, aperture (-1: none), p, seed, forward_only, and q, k, v, dctx: float32 arrays
(sum(lens), D) of seeded normal values ROUNDED TO bf16 (what the kernel reads).  scale = 0.06 throughout: logits of about N(0, 1) at D = 256."""
import numpy as np

from attn_strip_ref import bf16_round

SCALE = 0.06
# one video, D = 256: every NJ = ceil(T / 64) instance, every strip that ends inside a 32-key tile, the dummy tile slots (NJ = 1, 3, 5)
EDGE_T = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320)
RAGGED_N = (1, 7, 8, 9, 17)
WIDTHS = (512, 1024, 2048)
DROPOUT_P = (0.0, 0.1, 0.5, 0.9)


def _b(x):
    """x rounded to bf16, as a Python float"""
    return float(bf16_round(np.array([x], dtype=np.float32))[0])


def case(name, lens, D, seed, p=0.0, ignore_self=False, aperture=-1, drop_seed=None, forward_only=False):
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    q, k, v, dctx = (bf16_round(rng.standard_normal((n, D)).astype(np.float32)) for _ in range(4))
    return dict(name=name, lens=[int(t) for t in lens], D=D, scale=SCALE, ignore_self=bool(ignore_self), aperture=int(aperture), p=float(p),
                seed=int(seed * 7919 + 13 if drop_seed is None else drop_seed), forward_only=forward_only, q=q, k=k, v=v, dctx=dctx)


def edges():
    return [case(f"edge_T{T}", (T,), 256, 2000 + T) for T in EDGE_T]


def ragged_lens(n):
    """n lengths in 1 .. 320: the two ends, lengths on either side of a strip and of a key tile, the rest drawn."""
    fixed = (320, 1, 65, 33, 256, 2, 129, 64, 191)
    rng = np.random.default_rng(300 + n)
    lens = list(fixed[:n]) + [int(t) for t in rng.integers(1, 321, max(0, n - len(fixed)))]
    if n == 1:
        lens = [200]
    return lens


def ragged():
    return [case(f"ragged_n{n}", ragged_lens(n), 256, 3000 + n, p=0.5) for n in RAGGED_N]


def masks():
    lens = (70, 200, 33)
    out = [case("mask_ignore_self", lens, 256, 4001, ignore_self=True)]
    for ap in (0, 3, 400):
        out.append(case(f"mask_aperture{ap}", lens, 256, 4010 + ap % 97, aperture=ap))
        # (aperture 0 with ignore_self masks every key of every row: all NaN, nothing for a backward to read)
        out.append(case(f"mask_aperture{ap}_ignore_self", lens, 256, 4020 + ap % 97, aperture=ap, ignore_self=True, forward_only=ap == 0))
    out.append(case("mask_ignore_self_T1", (1,), 256, 4030, ignore_self=True, forward_only=True))
    out.append(case("mask_ignore_self_T1_in_batch", (5, 1, 66), 256, 4031, ignore_self=True, forward_only=True))
    return out


def width():
    return [case(f"width_D{D}", (65, 3, 320), D, 5000 + D, p=0.5) for D in WIDTHS]


LOUD_LENS = (200, 70)


def loud():
    """Column 0 of K is 1 and column 0 of a loud query row is c / scale: +c on every logit of that row (c = 30, and c = 100 where
    exp(logit) overflows float32 without the row maximum).  Column 1 of K is +40 / scale at ONE key of each video and -80 / scale at the
    others, column 1 of a saturating query row is 1: that key's weight is 1, the others' exp(-120 +- a few) underflow to 0."""
    c = case("loud", LOUD_LENS, 256, 6001)
    q, k = c["q"], c["k"]
    q[:, :2] = 0.0
    k[:, 0] = 1.0
    k[:, 1] = _b(-80.0 / SCALE)
    c["loud_keys"] = (197, 200 + 64)                          # inside the last partial 32-key tile of video 0; first key of video 1's second strip
    for j in c["loud_keys"]:
        k[j, 1] = _b(40.0 / SCALE)
    c["saturating_rows"] = (5, 67, 199, 200 + 3, 200 + 69)
    c["offset30_rows"] = (9, 130, 200 + 40)
    c["offset100_rows"] = (10, 131, 200 + 41)
    for r in c["saturating_rows"]:
        q[r, 1] = 1.0
    for r in c["offset30_rows"]:
        q[r, 0] = _b(30.0 / SCALE)
    for r in c["offset100_rows"]:
        q[r, 0] = _b(100.0 / SCALE)
    return [c]


def dropout():
    out = [case(f"dropout_p{p}", (129, 40), 256, 7000, p=p, drop_seed=11) for p in DROPOUT_P]
    out.append(case("dropout_p0.5_seed12", (129, 40), 256, 7000, p=0.5, drop_seed=12))
    return out


def families():
    return {"edges": edges(), "ragged": ragged(), "masks": masks(), "width": width(), "loud": loud(), "dropout": dropout()}
