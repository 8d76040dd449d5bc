"""Seeded input/weight recipes shared by the golden generator (make_golden.py, run once in the build
container against the real reference) and by the tests (which regenerate the same inputs anywhere).
numpy's PCG64 `default_rng` stream is platform independent, so full-size (D=1024) cases need only their
expected OUTPUTS committed, not 21 MB of weights."""
import hashlib
import numpy as np

VASNET_KEYS = ["K.weight", "Q.weight", "V.weight", "attention_head_projection.weight",
               "k1.weight", "k1.bias", "k2.weight", "k2.bias", "layer_norm.weight", "layer_norm.bias"]


def vasnet_weights(D, seed, max_length=None):
    """Xavier-like uniform matrices, non-trivial biases and LN affine (so the shared-LN quirk is exercised)."""
    rng = np.random.default_rng(seed)
    a = np.sqrt(2.0) * np.sqrt(6.0 / (2 * D))
    p = {}
    for k in ["K.weight", "Q.weight", "V.weight", "attention_head_projection.weight", "k1.weight"]:
        p[k] = rng.uniform(-a, a, (D, D)).astype(np.float32)
    p["k1.bias"] = rng.uniform(-0.2, 0.2, (D,)).astype(np.float32)
    p["k2.weight"] = rng.uniform(-a * 4, a * 4, (1, D)).astype(np.float32)
    p["k2.bias"] = rng.uniform(-0.2, 0.2, (1,)).astype(np.float32)
    p["layer_norm.weight"] = rng.uniform(0.5, 1.5, (D,)).astype(np.float32)
    p["layer_norm.bias"] = rng.uniform(-0.1, 0.1, (D,)).astype(np.float32)
    if max_length:
        p["pos_embed.weight"] = rng.normal(0, 1, (max_length, D)).astype(np.float32)
    return p


def lstm_weights(prefix, D, H, num_layers, seed, head_prefix):
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    p = {}
    for l in range(num_layers):
        In = D if l == 0 else 2 * H
        for suf in ("", "_reverse"):
            p[f"{prefix}weight_ih_l{l}{suf}"] = rng.uniform(-k, k, (4 * H, In)).astype(np.float32)
            p[f"{prefix}weight_hh_l{l}{suf}"] = rng.uniform(-k, k, (4 * H, H)).astype(np.float32)
            p[f"{prefix}bias_ih_l{l}{suf}"] = rng.uniform(-k, k, (4 * H,)).astype(np.float32)
            p[f"{prefix}bias_hh_l{l}{suf}"] = rng.uniform(-k, k, (4 * H,)).astype(np.float32)
    kh = 1.0 / np.sqrt(2 * H)
    p[f"{head_prefix}weight"] = rng.uniform(-kh * 3, kh * 3, (1, 2 * H)).astype(np.float32)
    p[f"{head_prefix}bias"] = rng.uniform(-kh, kh, (1,)).astype(np.float32)
    return p


def transformer_weights(D, n_layers, seed, max_length=None):
    """Weights of the reference Transformer scorer (state_dict keys of summarizer/models/transformer.py), seeded."""
    rng = np.random.default_rng(seed)
    a = np.sqrt(6.0 / (2 * D))
    u = lambda *shape, s=1.0: rng.uniform(-a * s, a * s, shape).astype(np.float32)
    p = {}
    for l in range(n_layers):
        pre = f"transformer_encoder.layers.{l}."
        p[pre + "self_attn.in_proj_weight"] = u(3 * D, D, s=1.5)
        p[pre + "self_attn.in_proj_bias"] = rng.uniform(-0.1, 0.1, (3 * D,)).astype(np.float32)
        p[pre + "self_attn.out_proj.weight"] = u(D, D)
        p[pre + "self_attn.out_proj.bias"] = rng.uniform(-0.1, 0.1, (D,)).astype(np.float32)
        p[pre + "linear1.weight"] = u(D, D, s=1.4); p[pre + "linear1.bias"] = rng.uniform(-0.1, 0.1, (D,)).astype(np.float32)
        p[pre + "linear2.weight"] = u(D, D, s=1.4); p[pre + "linear2.bias"] = rng.uniform(-0.1, 0.1, (D,)).astype(np.float32)
        for n in ("norm1", "norm2"):
            p[pre + n + ".weight"] = rng.uniform(0.7, 1.3, (D,)).astype(np.float32)
            p[pre + n + ".bias"] = rng.uniform(-0.1, 0.1, (D,)).astype(np.float32)
    p["layer_norm.weight"] = rng.uniform(0.7, 1.3, (D,)).astype(np.float32)
    p["layer_norm.bias"] = rng.uniform(-0.1, 0.1, (D,)).astype(np.float32)
    p["transformer_encoder.norm.weight"] = p["layer_norm.weight"]          # the same module registered twice
    p["transformer_encoder.norm.bias"] = p["layer_norm.bias"]
    p["k1.weight"] = u(D, D, s=1.4); p["k1.bias"] = rng.uniform(-0.2, 0.2, (D,)).astype(np.float32)
    p["k2.weight"] = u(1, D, s=4.0); p["k2.bias"] = rng.uniform(-0.2, 0.2, (1,)).astype(np.float32)
    if max_length:
        p["pos_embed.weight"] = rng.normal(0, 1, (max_length, D)).astype(np.float32)
    return p


def features(T, B, D, seed):
    """pool5-like non-negative features: 0.5*|N(0,1)|."""
    rng = np.random.default_rng(seed)
    return (0.5 * np.abs(rng.standard_normal((T, B, D)))).astype(np.float32)


def reward_features(kind, T, D, seed):
    """(T, D) float32 features on which BOTH terms of DSN's reward are visible in fp32.  With `features` as it is the squared distance
    between two frames grows with D (about 118 at D = 1024), so R_rep = exp(-mean min d2) underflows and a reward test compares R_div / 2
    alone.  Both kinds scale the features by 2.35 / sqrt(D): distances are O(1) for every D (about 1 between unrelated frames) and the
    cosine term is unchanged.
      "scaled": `features` times that scale.
      "shots":  a shot centre drawn like `features`, held for 8..16 frames (about 12), plus 0.05 N(0, 1) noise per frame: neighbouring
                frames are near duplicates, so d2 = G[t][t] + G[p][p] - 2 G[t][p] is a small difference of large Gram entries."""
    scale = np.float32(2.35 / np.sqrt(D))
    if kind == "scaled":
        return features(T, 1, D, seed)[:, 0, :] * scale
    if kind != "shots":
        raise KeyError(kind)
    rng = np.random.default_rng([seed, 77])
    rows = []
    while len(rows) < T:
        centre = 0.5 * np.abs(rng.standard_normal(D))
        rows += [centre] * int(rng.integers(8, 17))
    x = np.stack(rows[:T]) + 0.05 * rng.standard_normal((T, D))
    return x.astype(np.float32) * scale


def _reward_picks(rng, T, rate):
    """(T,) float32 0/1 actions at pick rate `rate` with at least one pick."""
    a = (rng.random(T) < rate).astype(np.float32)
    if not a.any():
        a[int(rng.integers(T))] = 1.0
    return a


REWARD_KINDS = ("scaled", "shots")
REWARD_TILE_T = (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 257, 320)      # T % 4 != 0: the Gram row pitch (T + 3) & ~3; 64 k +- 1: its 64 x 64 tiles
REWARD_TILE_D = (4, 8, 36, 100, 1024)                                   # D % 4 == 0 is required; 36 and 100 leave a K tail
REWARD_EPISODE_LENS = (60, 1, 37, 130, 64)
REWARD_FAMILIES = ("tiles", "isolation", "threshold", "many_videos", "episodes")


def reward_family(name):
    """The calls of one family of tests/test_gpu_reward_f64.py (tests/test_oracle.py checks on the float64 oracle that every one of them has
    a visible R_rep).  A call is a dict: id, lens, D, xs (one (T, D) float32 array per video), acts ((E, sum(lens)) float32), far_sim, thre,
    and for some families `expect`: {(episode, video): what the case isolates}."""
    calls = []

    def add(cid, xs, acts, thre=20, **extra):
        acts = np.ascontiguousarray(np.atleast_2d(acts), dtype=np.float32)
        if any(c["id"] == f"{cid}_far0" for c in calls):
            return
        for far in (False, True):
            calls.append(dict(id=f"{cid}_far{int(far)}", lens=[x.shape[0] for x in xs], D=xs[0].shape[1], xs=xs, acts=acts, far_sim=far,
                              thre=thre, **extra))

    if name == "tiles":                                             # one video per call: tile and padding edges of the Gram GEMM
        for ki, kind in enumerate(REWARD_KINDS):
            for D in REWARD_TILE_D:
                for T in REWARD_TILE_T:
                    x = reward_features(kind, T, D, 5000 + 13 * T + D)
                    for rate in (0.05, 0.4, 1.0):
                        rng = np.random.default_rng([T, D, int(rate * 100), ki])
                        add(f"{kind}_T{T}_D{D}_p{rate}", [x], _reward_picks(rng, T, rate))
    elif name == "isolation":                                       # one pick: R_div = 0, reward = R_rep / 2; every frame picked: R_rep = 1
        for kind in REWARD_KINDS:
            for T, D in ((3, 8), (64, 100), (129, 36), (320, 100)):
                x = reward_features(kind, T, D, 5100 + T + D)
                for where, t in (("first", 0), ("middle", T // 2), ("last", T - 1)):
                    a = np.zeros(T, np.float32)
                    a[t] = 1.0
                    add(f"{kind}_T{T}_D{D}_one_pick_{where}", [x], a, expect={(0, 0): "one_pick"})
                add(f"{kind}_T{T}_D{D}_all_picked", [x], np.ones(T, np.float32), expect={(0, 0): "all_picked"})
    elif name == "threshold":                                       # two picks `thre` and `thre + 1` frames apart, wherever a video of T = 70 has room
        T, D = 70, 36
        for kind in REWARD_KINDS:
            x = reward_features(kind, T, D, 5200)
            for thre in (0, 1, 20, T - 1, T + 5):
                for dist, first in ((thre, 0), (thre + 1, 0), (thre, T - 1 - thre), (thre + 1, T - 2 - thre), (thre, 7), (thre + 1, 11),
                                    (T - 1, 0)):
                    if dist < 1 or first < 0 or first + dist > T - 1:
                        continue
                    a = np.zeros(T, np.float32)
                    a[[first, first + dist]] = 1.0
                    add(f"{kind}_thre{thre}_picks{first}_{first + dist}", [x], a, thre=thre,
                        expect={(0, 0): "beyond_thre" if dist > thre else "within_thre"})
    elif name == "many_videos":                                     # the second and third block of reward_setup_kernel; the offset search over many videos
        D, E = 8, 3
        for kind in REWARD_KINDS:
            for n_seq in (64, 65, 130):
                rng = np.random.default_rng([n_seq, REWARD_KINDS.index(kind)])
                lens = [int(t) for t in rng.integers(1, 10, n_seq)]
                if n_seq == 130:
                    lens[70] = 129                                  # one long video behind the first block's 64
                xs = [reward_features(kind, T, D, 5300 + 7 * i + n_seq) for i, T in enumerate(lens)]
                acts = np.concatenate([np.stack([_reward_picks(rng, T, 0.7) for _ in range(E)]) for T in lens], axis=1)
                add(f"{kind}_n{n_seq}", xs, acts)
    elif name == "episodes":                                        # E episodes of a ragged batch in one call
        D = 36
        for kind in REWARD_KINDS:
            xs = [reward_features(kind, T, D, 5400 + i) for i, T in enumerate(REWARD_EPISODE_LENS)]
            off = np.concatenate([[0], np.cumsum(REWARD_EPISODE_LENS)])
            for E in (1, 5, 9):
                rng = np.random.default_rng([E, REWARD_KINDS.index(kind)])
                acts = np.concatenate([np.stack([_reward_picks(rng, T, (0.4, 0.1, 0.7)[e % 3]) for e in range(E)]) for T in REWARD_EPISODE_LENS], axis=1)
                expect = {}
                # action values other than 1.0 are picks too, -0.0 is none (episode 0 of every E)
                picked = np.flatnonzero(acts[0])
                acts[0, picked[0::3]] = 2.0
                acts[0, picked[1::3]] = -1.0
                acts[0, np.flatnonzero(acts[0] == 0)[::2]] = -0.0
                if E >= 5:
                    acts[1, :] = 0.0                                # nothing picked anywhere: reward exactly 0
                    acts[1, ::3] = -0.0
                    acts[2, :] = 0.0                                # one pick per video
                    for s, T in enumerate(REWARD_EPISODE_LENS):
                        acts[2, off[s] + (7 * s) % T] = 1.0
                    acts[3, :] = 1.0                                # every frame picked
                    for s in range(len(REWARD_EPISODE_LENS)):
                        expect.update({(1, s): "no_pick", (2, s): "one_pick", (3, s): "all_picked"})
                add(f"{kind}_E{E}", xs, acts, expect=expect)
    else:
        raise KeyError(name)
    return calls


POLICY_BATCHES = ("ragged", "short")
POLICY_CLAMP = np.float32(np.finfo(np.float32).eps)                 # clamp_probs of torch.distributions in fp32


def policy_case(batch, E):
    """Inputs of the REINFORCE loss kernels for tests/test_gpu_reward_f64.py: dict(lens, probs (R,), actions (E, R), rewards (E, V), base (V,),
    dlv (V,), outside: rows whose probability lies outside the clamp).  All float32.
      "ragged": T = 1, 255, 256, 257, 513, 1100 -- one to five passes of the kernels' 256-frame stride; "short": 70 videos of 1..9 frames.
    The inputs are WELL CONDITIONED on purpose, so that the float64 comparison measures the kernels' rounding and not a cancellation that the
    fp32 yardstick would share only by chance:
      * probabilities of a video lie in [0.02, 0.3] (even videos) or [0.7, 0.98] (odd videos), so mean p - 0.5 (target 0.5) keeps at least
        0.2 of its operands' size -- the length penalty's gradient 2 beta (mean p - eps) is the WHOLE gradient outside the clamp;
      * per video the advantages r - b are all positive (baseline 0.1 under rewards in [0.3, 0.8]), all negative (baseline 2.0: beyond the length penalty at beta = 1, which has the other sign) or, for every
        third video without a special probability (E >= 3), positive but for one episode (reward 0.05 under a baseline of 0.25).
    Special probabilities sit on their video's side: 0, eps, one ulp below eps, 1e-9 in low videos; 1, 1 - eps, one ulp above 1 - eps in high
    ones -- in the ragged batch behind the first, second and fourth 256-frame pass as well as in front.  The upstream gradient has both signs
    and is exactly 0 for every fifth video."""
    c = POLICY_CLAMP
    below, above = np.nextafter(c, np.float32(0)), np.nextafter(np.float32(1) - c, np.float32(1))
    if batch == "ragged":
        lens = [1, 255, 256, 257, 513, 1100]
        special = {2: {255: 0.0}, 3: {256: 1.0, 0: np.float32(1) - c},
                   4: {2: 0.0, 256: c, 400: below, 512: 1e-9, 511: c}, 5: {3: 1.0, 300: np.float32(1) - c, 600: above, 1099: 1.0, 1024: np.float32(1) - c}}
    elif batch == "short":
        rng_t = np.random.default_rng(41)
        lens = [int(t) for t in rng_t.integers(1, 10, 70)]
        lens[0], lens[3] = 1, 1                                     # a video that is one clamped frame: no log-prob gradient at all
        special = {0: {0: 0.0}, 3: {0: 1.0}, 4: {0: c}, 7: {lens[7] - 1: np.float32(1) - c}, 12: {0: 1e-9}, 65: {0: above}, 68: {lens[68] - 1: below}}
    else:
        raise KeyError(batch)
    V, off = len(lens), np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng([E, POLICY_BATCHES.index(batch), 9])
    probs = np.empty(off[-1], np.float32)
    for v in range(V):
        lo = 0.02 if v % 2 == 0 else 0.7
        probs[off[v]:off[v + 1]] = rng.uniform(lo, lo + 0.28, lens[v]).astype(np.float32)
        for t, val in special.get(v, {}).items():
            probs[off[v] + t] = np.float32(val)
    actions = (rng.random((E, off[-1])) < 0.4).astype(np.float32)
    rewards = rng.uniform(0.3, 0.8, (E, V)).astype(np.float32)
    base = np.empty(V, np.float32)
    for v in range(V):
        pattern = v % 3 if v not in special and E >= 3 else v % 2
        base[v] = (0.1, 2.0, 0.25)[pattern]
        if pattern == 2:
            rewards[v % E, v] = 0.05
    dlv = (rng.uniform(0.5, 1.5, V) * np.where(rng.random(V) < 0.5, -1.0, 1.0)).astype(np.float32)
    dlv[1::5] = 0.0
    outside = np.flatnonzero((probs < c) | (probs > np.float32(1) - c))
    return dict(lens=lens, probs=probs, actions=actions, rewards=rewards, base=base, dlv=dlv, outside=outside)


def digest(arrs):
    h = hashlib.sha256()
    for k in sorted(arrs):
        h.update(k.encode()); h.update(np.ascontiguousarray(arrs[k]).tobytes())
    return h.hexdigest()


def synthetic_video(T, seed, n_users=15, D=None):
    """SumMe/TVSum-shaped evaluation metadata: picks every 15th frame, random change points."""
    rng = np.random.default_rng(seed)
    n_frames = int(15 * T - rng.integers(0, 15))
    picks = (15 * np.arange(T)).astype(np.int32)
    n_seg = max(1, T // 15)
    cuts = np.sort(rng.choice(np.arange(15, n_frames - 15), size=n_seg - 1, replace=False)) if n_seg > 1 else np.array([], int)
    starts = np.concatenate([[0], cuts]).astype(np.int64)
    ends = np.concatenate([cuts - 1, [n_frames - 1]]).astype(np.int64)
    cps = np.stack([starts, ends], axis=1).astype(np.int32)
    nfps = (ends - starts + 1).astype(np.int32)
    user_summary = (rng.random((n_users, n_frames)) < 0.15).astype(np.float32)
    gt = rng.random((T + 1) // 2).repeat(2)[:T].astype(np.float32)
    user_scores = np.clip(gt[None, :] + 0.3 * rng.standard_normal((n_users, T)), 0, 1).astype(np.float32)
    user_scores_frames = np.repeat(user_scores, 15, axis=1)[:, :n_frames]
    if user_scores_frames.shape[1] < n_frames:
        user_scores_frames = np.pad(user_scores_frames, ((0, 0), (0, n_frames - user_scores_frames.shape[1])))
    d = dict(n_frames=n_frames, picks=picks, change_points=cps, n_frame_per_seg=nfps,
             user_summary=user_summary, gtscore=gt, user_scores=user_scores_frames.astype(np.float32))
    if D:
        d["features"] = features(T, 1, D, seed + 7)[:, 0, :]
    return d


# ---- evaluation-tail geometries the plain synthetic_video never has (tests/test_oracle.py shows each edge is present; tests/test_gpu_evaltail.py
# runs them on the device).  Every edge keeps picks ascending and at most 4096 of them: the videos stay eligible for the device tail.
EVAL_EDGES = ("picks_from_7", "picks_from_15", "last_pick_is_n_frames", "repeated_picks", "one_more_interval", "cps_start_below_0",
              "cps_end_past_video", "segment_lengths", "pick_spacing_2", "n_frames_1", "n_frames_5", "n_frames_9")
EDGE_SEGMENT_LENGTHS = (1, 7, 8, 9, 128, 129, 257, 1100)      # numpy's pairwise sum: < 8 plain loop, <= 128 one block, above: split once, ... , split 4 times


def edge_video(v, edge):
    """`v` (a synthetic_video dict, or the result of an earlier edge_video: edges combine) with one named edge of the evaluation geometry
    applied.  The result carries "n_steps", the number of scores the video is evaluated with; annotator data is redrawn for the new length."""
    import zlib
    if edge not in EVAL_EDGES:
        raise KeyError(edge)
    picks = np.asarray(v["picks"]).astype(np.int64).copy()
    cps = np.asarray(v["change_points"]).astype(np.int64).copy()
    n_frames, n_steps = int(v["n_frames"]), int(v.get("n_steps", len(picks)))
    n_users = v["user_summary"].shape[0]
    rng = np.random.default_rng([zlib.crc32(edge.encode()), n_frames, n_users])
    step = int(picks[-1] - picks[-2]) if len(picks) > 1 and picks[-1] > picks[-2] else 15
    if edge in ("picks_from_7", "picks_from_15"):                    # frames in front of the first pick: covered by no interval, value 0
        k = 7 if edge == "picks_from_7" else 15
        picks += k; n_frames += k; cps += k; cps[0, 0] = 0
    elif edge == "last_pick_is_n_frames":                            # no sentinel appended (eval.py:27-28): n_picks - 1 intervals
        n_frames = int(picks[-1]) + step
        picks = np.append(picks, n_frames)
        cps[-1, 1] = n_frames - 1
    elif edge == "repeated_picks":                                   # empty intervals: a run of 2 and a run of 3 equal picks
        assert len(picks) >= 10
        picks[3] = picks[2]
        picks[8] = picks[9] = picks[7]
    elif edge == "one_more_interval":                                # n_int == n_steps + 1: the last interval has no score and takes 0 (eval.py:31-32)
        picks = np.append(picks, picks[-1] + step)
        n_frames = int(picks[-1]) + 9
        cps[-1, 1] = n_frames - 1
    elif edge == "cps_start_below_0":
        cps[0, 0] = -5
    elif edge == "cps_end_past_video":
        cps[-1, 1] = n_frames + 10
    elif edge == "segment_lengths":
        assert n_frames > sum(EDGE_SEGMENT_LENGTHS) + 16
        starts = np.concatenate([[0], np.cumsum(EDGE_SEGMENT_LENGTHS)])
        ends = np.concatenate([starts[1:] - 1, [n_frames - 1]])
        cps = np.stack([starts, ends], axis=1)
    elif edge == "pick_spacing_2":                                   # thousands of scoring steps in a video of ~2 x n_steps frames
        picks = 2 * np.arange(n_steps, dtype=np.int64)
        n_frames = 2 * n_steps + 1
        cuts = np.sort(rng.choice(np.arange(8, n_frames - 8), size=max(1, n_frames // 100) - 1, replace=False))
        cps = np.stack([np.concatenate([[0], cuts]), np.concatenate([cuts - 1, [n_frames - 1]])], axis=1)
    else:                                                            # n_frames_1 / _5 / _9: fewer frames than a thread block, a wave, a chunk
        n_frames = int(edge.rsplit("_", 1)[1])
        picks = np.arange(0, n_frames, 4, dtype=np.int64)
        n_steps = len(picks)
        cps = np.array([[0, n_frames - 1]], dtype=np.int64)
    lo, hi = np.clip(cps[:, 0], 0, n_frames), np.clip(cps[:, 1] + 1, 0, n_frames)
    nfps = np.maximum(hi - lo, 0).astype(np.int32)
    user_summary = (rng.random((n_users, n_frames)) < 0.15).astype(np.float32)
    coarse = rng.random((n_users, (n_frames + 14) // 15)).astype(np.float32)
    user_scores = np.repeat(coarse, 15, axis=1)[:, :n_frames].copy()
    if n_frames < 30:                                                # (one or two constant stretches would leave the annotators' ranks all tied)
        user_scores = rng.random((n_users, n_frames)).astype(np.float32)
    return dict(n_frames=n_frames, picks=picks.astype(np.int32), change_points=cps.astype(np.int32), n_frame_per_seg=nfps,
                user_summary=user_summary, user_scores=user_scores, n_steps=n_steps)


def edge_scores(kind, n_steps, seed):
    """Step scores for the evaluation edges: "random" in [0, 1); "zeros": every third score exactly 0.0 (ties with frames no interval covers);
    "negative": signed scores with some +0.0 and -0.0; "all_zero": every score 0.0."""
    rng = np.random.default_rng(seed)
    s = rng.random(n_steps).astype(np.float32)
    if kind == "zeros":
        s[::3] = 0.0
    elif kind == "negative":
        s = rng.standard_normal(n_steps).astype(np.float32)
        s[1::5] = np.float32(-0.0)
        s[3::7] = np.float32(0.0)
    elif kind == "all_zero":
        s[:] = np.float32(0.0)
    elif kind != "random":
        raise KeyError(kind)
    return s


def eval_edge_batch():
    """The edge batch of tests/test_oracle.py (host tail vs the numpy oracle) and tests/test_gpu_evaltail.py (device tail vs both): one
    video per edge plus two that combine edges; annotator counts 1, 2, 31, 32.  Returns [(name, video dict, scores (n_steps,) float32)]."""
    spec = [  # (name, base n_steps, annotators, edges, scores)
        ("picks_from_7", 60, 1, ["picks_from_7"], "random"),
        ("picks_from_15+zeros", 45, 2, ["picks_from_15"], "zeros"),
        ("last_pick_is_n_frames", 80, 31, ["last_pick_is_n_frames"], "random"),
        ("repeated_picks", 50, 32, ["repeated_picks"], "random"),
        ("one_more_interval", 40, 2, ["one_more_interval"], "random"),
        ("cps_start_below_0", 70, 31, ["cps_start_below_0"], "random"),
        ("cps_end_past_video", 70, 32, ["cps_end_past_video"], "random"),
        ("segment_lengths", 130, 1, ["segment_lengths"], "random"),
        ("steps_4000", 4000, 2, ["pick_spacing_2"], "random"),
        ("steps_4095", 4095, 31, ["pick_spacing_2"], "negative"),
        ("n_frames_1", 1, 32, ["n_frames_1"], "random"),
        ("n_frames_5", 2, 1, ["n_frames_5"], "random"),
        ("n_frames_9", 3, 2, ["n_frames_9"], "random"),
        ("negative_scores", 90, 31, [], "negative"),
        ("picks_from_7+repeated_picks+zeros", 55, 32, ["picks_from_7", "repeated_picks"], "zeros"),
        ("steps_4095+one_more_interval", 4095, 1, ["pick_spacing_2", "one_more_interval"], "random"),     # 4096 intervals: the device limit
        ("all_zero+picks_from_7", 33, 2, ["picks_from_7"], "all_zero"),      # every interval ties with the uncovered frames: one rank group, NaN
    ]
    out = []
    for i, (name, T, U, edges, kind) in enumerate(spec):
        if T > 1000:                                                # (only the length and the annotator count of the base video survive pick_spacing_2)
            v = dict(n_frames=15 * T, picks=(15 * np.arange(T)).astype(np.int32), change_points=np.array([[0, 15 * T - 1]], np.int32),
                     user_summary=np.zeros((U, 1), np.float32))
        else:
            v = synthetic_video(max(T, 1), 8300 + i, n_users=U)
        v = dict(v, n_steps=T)
        for e in edges:
            v = edge_video(v, e)
        out.append((name, v, edge_scores(kind, v["n_steps"], 8400 + i)))
    return out


def dropout_keep(seed, site, idx, p):
    """numpy twin of sumk::dropout_keep (csrc/sumk_internal.h): keep-mask of training-mode dropout as a pure
    function of (seed, site, element index).  idx: uint64 array.  Returns a bool array (True = kept)."""
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) ^ (np.uint64(site + 1) * np.uint64(0x9E3779B97F4A7C15))) + idx * np.uint64(0xD1342543DE82EF95)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    thr = min(int(float(np.float32(p)) * 4294967296.0), 0xFFFFFFFF)
    return (z >> np.uint64(32)).astype(np.uint64) >= np.uint64(thr)


def vasnet_drop_masks(seed, p, lens, D):
    """Scaled keep-masks (0 or 1/(1-p)) of the three dropout sites for a packed batch, per video:
    returns list of (m_alpha (T,T), m_y (T,D), m_z (T,D)) float32, indexed exactly like the HIP kernels."""
    sc = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    out, row0 = [], 0
    for T in lens:
        rows = (np.arange(T, dtype=np.uint64) + np.uint64(row0))
        ia = (rows[:, None] << np.uint64(20)) | np.arange(T, dtype=np.uint64)[None, :]
        iy = rows[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None, :]
        out.append(tuple((dropout_keep(seed, site, ix, p).astype(np.float32) * sc) for site, ix in ((0, ia), (1, iy), (2, iy))))
        row0 += T
    return out


def _scaled_keep(seed, p, site, idx):
    """Scaled keep-mask (0 or 1/(1-p), float32) of one dropout site at the element indices idx (uint64 array)."""
    sc = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return dropout_keep(seed, site, idx, p).astype(np.float32) * sc


def _flat_idx(R, N):
    """row * N + col over a packed (R, N) matrix: the GEMM epilogue's dropout index."""
    return np.arange(R, dtype=np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]


def _attn_masks(seed, p, site, lens, heads):
    """[(heads, T, T) per video]: index ((row*heads + h) << 20) | j with `row` the packed query row (tf_softmax_kernel)."""
    rows = np.arange(int(sum(lens)), dtype=np.uint64)
    per_video, r0 = [], 0
    for T in lens:
        wid = (rows[r0:r0 + T][None, :] * np.uint64(heads) + np.arange(heads, dtype=np.uint64)[:, None])      # (heads, T)
        per_video.append(_scaled_keep(seed, p, site, (wid[:, :, None] << np.uint64(20)) | np.arange(T, dtype=np.uint64)[None, None, :]))
        r0 += T
    return per_video


def transformer_drop_masks(seed, p_layer, p_head, lens, D, F, heads, n_layers):
    """Scaled keep-masks (0 or 1/(1-p)) of every dropout site of the Transformer scorer's training forward for a packed batch, in the
    layout oracle/torch_port.transformer_ref takes: {"attn": [[(heads, T, T) per video] per layer], "out": [(R, D)], "ff1": [(R, F)],
    "ff2": [(R, D)] per layer, "head": (R, D)}, float32.  `seed` is sumk_tf_opts.seed.  Index conventions, as the kernels compute them
    (`row` is always the PACKED row):
      site 10*l + 0  attention probabilities   ((row*heads + h) << 20) | j    csrc/transformer.hip tf_softmax_kernel (wid = row*heads + h)
      site 10*l + 1  out-proj (dropout1)       row * D + col                  csrc/gemm_device.h:22 (GEMM epilogue), tf_sa_fwd site + 1
      site 10*l + 2  linear1 after ReLU        row * F + col                  same epilogue (EPI_BIAS_RELU), tf_ff_fwd site_a
      site 10*l + 3  linear2 (dropout2)        row * D + col                  same epilogue (EPI_BIAS_RESIDUAL), tf_ff_fwd site_b
      site 1000      after ReLU(k1)            row * D + col                  csrc/vasnet.hip launch_ln_rows (layernorm_kernel, drop.thr branch)"""
    out = tf_stack_drop_masks(seed, p_layer, lens, D, F, heads, n_layers, decoder=False)
    out["head"] = _scaled_keep(seed, p_head, 1000, _flat_idx(int(sum(lens)), D))
    return out


def tf_stack_drop_masks(seed, p, lens, D, F, heads, n_layers, decoder):
    """Scaled keep-masks (0 or 1/(1-p), float32) of every dropout site of the SumGAN-Att stacks' training forward
    (csrc/tf_decoder.hip: sumk_tf_encoder_forward / sumk_tf_decoder_forward, site = 10 * l) for a packed batch, in the layout
    oracle/torch_port.tf_encoder_stack_ref / tf_decoder_stack_ref take.  `seed` is sumk_tf_opts.seed, p its layer_dropout_p.
    Sites +0 .. +3 are transformer_drop_masks' (the same blocks: tf_sa_fwd, tf_ff_fwd); with decoder=True also (`row` = PACKED row):
      "cattn" [[(heads, T, T) per video] per layer]  site 10*l + 4  cross-attention weights    ((row*heads + h) << 20) | j
            csrc/transformer.hip tf_softmax_kernel (wid = row*heads + h) via tf_attn_core_fwd(..., site + 4) in
            sumk_tf_decoder_forward; the backward draws the same index in tf_softmax_bwd_kernel via tf_attn_core_bwd(..., site + 4)
      "cout"  [(R, D) per layer]                     site 10*l + 5  cross out-proj (dropout2)  row * D + col
            csrc/gemm_device.h GEMM epilogue (EPI_BIAS_RESIDUAL: row * N + col, N = D) via tf_out_proj(..., site + 5); the backward
            is mask_scale_kernel (csrc/transformer.hip: flat index i = row * D + col) launched by sumk_tf_decoder_backward at site + 5"""
    R = int(sum(lens))
    out = {"attn": [], "out": [], "ff1": [], "ff2": []}
    if decoder:
        out.update(cattn=[], cout=[])
    for l in range(n_layers):
        site = 10 * l
        out["attn"].append(_attn_masks(seed, p, site, lens, heads))
        out["out"].append(_scaled_keep(seed, p, site + 1, _flat_idx(R, D)))
        out["ff1"].append(_scaled_keep(seed, p, site + 2, _flat_idx(R, F)))
        out["ff2"].append(_scaled_keep(seed, p, site + 3, _flat_idx(R, D)))
        if decoder:
            out["cattn"].append(_attn_masks(seed, p, site + 4, lens, heads))
            out["cout"].append(_scaled_keep(seed, p, site + 5, _flat_idx(R, D)))
    return out


class DetRandom:
    """Counter-based stand-in for torch.randn_like / torch.rand, used to run the reference's SumGAN trainer and the HIP one
    on the SAME draws (their generators -- torch CPU vs device -- cannot be matched): draw n comes from
    numpy.random.default_rng([seed, n]) whatever the device."""

    def __init__(self, seed):
        self.seed, self.n = int(seed), 0

    def _next(self, shape, kind):
        import torch
        self.n += 1
        g = np.random.default_rng([self.seed, self.n])
        a = g.standard_normal(tuple(shape)) if kind == "normal" else g.random(tuple(shape))
        return torch.from_numpy(a.astype(np.float32))

    def randn_like(self, t, **kw):
        return self._next(t.shape, "normal").to(t.device)

    def rand(self, *size, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list)):
            size = tuple(size[0])
        out = self._next(size, "uniform")
        return out.to(kw["device"]) if kw.get("device") is not None else out

    def patch(self):
        """Context manager: torch.randn_like / torch.rand -> this generator."""
        import contextlib
        import torch

        @contextlib.contextmanager
        def cm():
            old = torch.randn_like, torch.rand
            torch.randn_like, torch.rand = self.randn_like, self.rand
            try:
                yield self
            finally:
                torch.randn_like, torch.rand = old
        return cm()


def sample_idx(name, numel, n=256):
    """Flat indices at which a large tensor is digested (train_full.npz): seeded by the parameter name, sorted, unique."""
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")
    return np.sort(np.random.default_rng(seed).choice(numel, size=min(n, numel), replace=False))
