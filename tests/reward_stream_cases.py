"""Cases and the float64 gate of the streaming DSN reward (csrc/reward_stream.hip), shared by tests/test_gpu_reward_stream.py (GPU) and
tests/test_reward_stream_host.py (CPU: the recipe conditions on the oracle alone).  No kernel is involved in anything here.

The gate is that of tests/test_gpu_reward_f64.py: the reference is oracle/reward_np.reward_terms in float64; the yardstick of a family
is the largest |fp32 oracle - float64 oracle| over its cases (the fp32 side is the ORACLE run in fp32, not a restatement of the kernel's
summation order: the kernel accumulates its row and block sums in a fixed tree and the last join in float64, which is no larger); the
gate is 4 x the yardstick, with a floor of 2 fp32 ulps of the value.  Features come from `recipes.reward_features`, so R_rep >= 0.2 in
every compared case and both terms of a reward stand five orders of magnitude above the gate.

A call is a dict as `recipes.reward_family` builds it: id, lens, D, xs, acts (E, sum(lens)), far_sim, thre and, for some, `expect`:
{(episode, video): "no_pick" | "one_pick" | "all_picked" | "beyond_thre" | "within_thre"}."""
import functools

import numpy as np

import recipes as R
from oracle import reward_np

ULP = 2.0 ** -24
EC = 8                                     # episodes per pass of the kernel (kernels.REWARD_STREAM_EC; the GPU test asserts they agree)
OLD_FAMILIES = R.REWARD_FAMILIES           # tiles, isolation, threshold, many_videos, episodes: run through path="stream" as they are
NEW_FAMILIES = ("strips", "splits", "chunks", "tile_edges", "skipped", "offsets", "zero_norm")
STRIP_T = (65, 129, 191, 192, 193, 257, 700)          # one, two, three, four (minus one / exact / plus one), five and eleven 64-row strips
STRIP_D = (8, 36, 100)                                # one k-tile with a tail, two with a tail, four with a tail
RAGGED = (60, 1, 193, 130, 64)
SPLIT_T = (193, 700)
SPLITS = (1, 2, 3, 8)                                 # 8 is more than the four column tiles of T = 193
CHUNK_E = (1, EC - 1, EC, EC + 1, 2 * EC + 1)
EDGE_PAIRS = ((31, 32), (63, 64), (63, 84), (64, 84))  # across the 32-key sub-tile edge, across the tile edge, 21 and 20 apart over it
EDGE_THRE = (0, 1, 20, 21)
FILLER_T = (1 << 19) + 64                             # x (FILLER_T, 1024) fp32 is 2^31 + 2^18 bytes: the next video lies past 2^31 bytes
OFFSET_T, OFFSET_D = 130, 1024


def _calls(name):
    calls = []

    def add(cid, xs, acts, thre=20, **extra):
        acts = np.ascontiguousarray(np.atleast_2d(acts), dtype=np.float32)
        for far in (False, True):
            calls.append(dict(id=f"{cid}_far{int(far)}", lens=[x.shape[0] for x in xs], D=xs[0].shape[1], xs=xs, acts=acts, far_sim=far,
                              thre=thre, **extra))

    if name in OLD_FAMILIES:
        return R.reward_family(name)
    if name == "strips":
        for ki, kind in enumerate(R.REWARD_KINDS):
            for D in STRIP_D:
                for T in STRIP_T:
                    rng = np.random.default_rng([T, D, ki, 61])
                    add(f"{kind}_T{T}_D{D}", [R.reward_features(kind, T, D, 6000 + 3 * T + D)], R._reward_picks(rng, T, 0.4))
            xs = [R.reward_features(kind, T, 36, 6100 + i) for i, T in enumerate(RAGGED)]
            rng = np.random.default_rng([ki, 62])
            add(f"{kind}_ragged", xs, np.concatenate([np.stack([R._reward_picks(rng, T, (0.4, 0.1, 0.7)[e]) for e in range(3)]) for T in RAGGED], axis=1))
    elif name == "splits":
        for ki, kind in enumerate(R.REWARD_KINDS):
            for T in SPLIT_T:
                rng = np.random.default_rng([T, ki, 63])
                add(f"{kind}_T{T}", [R.reward_features(kind, T, 36, 6200 + T)], np.stack([R._reward_picks(rng, T, r) for r in (0.5, 0.05, 1.0)]))
    elif name == "chunks":
        lens = (70, 130)
        for ki, kind in enumerate(R.REWARD_KINDS):
            xs = [R.reward_features(kind, T, 36, 6300 + i) for i, T in enumerate(lens)]
            for E in CHUNK_E:
                rng = np.random.default_rng([E, ki, 64])
                acts = np.concatenate([np.stack([R._reward_picks(rng, T, (0.4, 0.1, 0.7)[e % 3]) for e in range(E)]) for T in lens], axis=1)
                expect = {}
                if E >= 3:
                    acts[1, :] = 0.0                                    # an episode without picks ...
                    acts[E - 1, :] = 1.0                                # ... and one that picks everything (the last: alone in its chunk for E = EC + 1, 2 EC + 1)
                    for s in range(len(lens)):
                        expect.update({(1, s): "no_pick", (E - 1, s): "all_picked"})
                add(f"{kind}_E{E}", xs, acts, expect=expect)
    elif name == "tile_edges":
        T, D = 100, 36
        for kind in R.REWARD_KINDS:
            x = R.reward_features(kind, T, D, 6400)
            for thre in EDGE_THRE:
                for p, q in EDGE_PAIRS:
                    a = np.zeros(T, np.float32)
                    a[[p, q]] = 1.0
                    add(f"{kind}_thre{thre}_picks{p}_{q}", [x], a, thre=thre, expect={(0, 0): "beyond_thre" if q - p > thre else "within_thre"})
    elif name == "skipped":
        T, D = 300, 36                                                  # five column tiles
        for ki, kind in enumerate(R.REWARD_KINDS):
            x = R.reward_features(kind, T, D, 6500)
            rng = np.random.default_rng([ki, 65])
            last, first = np.zeros(T, np.float32), np.zeros(T, np.float32)
            last[256:] = R._reward_picks(rng, T - 256, 0.4)
            first[:64] = R._reward_picks(rng, 64, 0.4)
            add(f"{kind}_last_tile_only", [x], last)
            add(f"{kind}_first_tile_only", [x], first)
            alone = np.zeros((3, T), np.float32)                        # every tile that is walked has picks in ONE episode of the chunk alone
            alone[0, 64:128] = R._reward_picks(rng, 64, 0.4)
            alone[1, 192:256] = R._reward_picks(rng, 64, 0.4)
            add(f"{kind}_one_episode_per_tile", [x], alone, expect={(2, 0): "no_pick"})
    elif name == "offsets":                                             # the video BEHIND the filler; the GPU test puts the filler in front of it
        for ki, kind in enumerate(R.REWARD_KINDS):
            rng = np.random.default_rng([ki, 66])
            add(f"{kind}_behind_filler", [R.reward_features(kind, OFFSET_T, OFFSET_D, 6600)],
                np.stack([R._reward_picks(rng, OFFSET_T, r) for r in (0.5, 0.1, 0.9, 0.5, 0.3)]))
    elif name == "zero_norm":
        # as tests/test_gpu_reward_f64.py::zero_norm_calls: the middle video has one all-zero feature row (frame 17).  Episode 0 picks it among
        # others, episode 1 leaves it out, episode 2 picks it alone (one pick: no cosine is taken), episode 3 picks every frame.
        lens, D, z = [9, 40, 5], 8, 17
        for kind in R.REWARD_KINDS:
            xs = [R.reward_features(kind, T, D, 5600 + i).copy() for i, T in enumerate(lens)]
            xs[1][z] = 0.0
            rng = np.random.default_rng(56)
            acts = (rng.random((4, sum(lens))) < 0.4).astype(np.float32)
            acts[:, [0, 9 + 3, 9 + 30, 9 + 40]] = 1.0
            acts[0, 9 + z], acts[1, 9 + z] = 1.0, 0.0
            acts[2, 9:9 + 40] = 0.0
            acts[2, 9 + z] = 1.0
            acts[3, :] = 1.0
            add(f"zero_norm_{kind}", xs, acts, thre=5)
    else:
        raise KeyError(name)
    return calls


ZERO_NORM_NAN = np.zeros((4, 3), bool)
ZERO_NORM_NAN[0, 1] = ZERO_NORM_NAN[3, 1] = True


def oracle(calls):
    """[(terms64 (E, S, 3), reward32 (E, S))] per call and the yardstick: the largest |fp32 oracle - float64 oracle| over all of them."""
    refs, yard = [], 0.0
    for call in calls:
        off = np.concatenate([[0], np.cumsum(call["lens"])])
        E, S = call["acts"].shape[0], len(call["lens"])
        t64, r32 = np.zeros((E, S, 3)), np.zeros((E, S))
        for e in range(E):
            for s, x in enumerate(call["xs"]):
                a = call["acts"][e, off[s]:off[s + 1]]
                t64[e, s] = reward_np.reward_terms(x, a, call["far_sim"], call["thre"], np.float64)
                r32[e, s] = reward_np.compute_reward(x, a, call["far_sim"], call["thre"], np.float32)
        fin = np.isfinite(t64[:, :, 2])
        assert np.array_equal(fin, np.isfinite(r32))
        if fin.any():
            yard = max(yard, float(np.abs(r32 - t64[:, :, 2])[fin].max()))
        refs.append((t64, r32))
    return refs, yard


@functools.lru_cache(maxsize=None)
def family(name):
    """(calls, refs, yardstick) of one family, computed once and left unchanged."""
    calls = _calls(name)
    refs, yard = oracle(calls)
    return calls, refs, yard


def gate(yard, ref):
    return 4 * max(yard, 2 * ULP * abs(ref))


def compare(call, got, t64, yard, skip=None):
    """Every (episode, video) of one call against the float64 terms.  Returns (worst error / yardstick, [failures]).  skip: a bool (E, S)
    array of results that are judged elsewhere (the NaN rewards of the zero-norm family)."""
    worst, bad = 0.0, []
    expect = call.get("expect", {})
    for e in range(got.shape[0]):
        for s in range(got.shape[1]):
            if skip is not None and skip[e, s]:
                continue
            g = float(got[e, s])
            r_div, r_rep, ref = t64[e, s]
            what = expect.get((e, s))
            if what == "no_pick" or (what is None and ref == 0.0 and r_rep == 0.0):      # dsn.py:199-203: exactly 0
                if g != 0.0 or np.signbit(g):
                    bad.append((call["id"], e, s, "no_pick", g))
                continue
            y = max(yard, 2 * ULP * abs(ref))
            errs = {"reward": abs(g - ref)}
            if what == "one_pick":
                errs["2r_vs_r_rep"] = abs(2 * g - r_rep)
            elif what == "all_picked":
                errs["2r-1_vs_r_div"] = abs(2 * g - 1 - r_div)
            elif what in ("beyond_thre", "within_thre"):
                errs["2r-r_rep_vs_r_div"] = abs(2 * g - r_rep - r_div)
            for k, err in errs.items():
                worst = max(worst, err / y)
                if not err <= 4 * y:
                    bad.append((call["id"], e, s, what, k, g, ref, err, y))
    return worst, bad
