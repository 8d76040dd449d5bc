"""Transformer-encoder scorer on MI355X -- drop-in for `summarizer/models/transformer.py` (reference): model class and
trainer (the first "next" model after the north_star scorers).

Same constructor (transformer.py:19), same parameter names / state_dict keys (the stock `nn.TransformerEncoder` objects are
kept as PARAMETER CONTAINERS and never called), same forward contract x (seq_len, batch, input_size) -> (seq_len, batch, 1).
Quirks reproduced: one `layer_norm` used as the encoder's final norm AND after k1 (transformer.py:47,50,100); the in-place
positional add with the sinusoid table's batch re-view (transformer.py:83-89).  Training runs through HIP backward kernels;
its dropouts (0.1 inside the encoder layers, 0.5 after k1) use the deterministic hash masks of the VASNet path.
"""
import math
import random
import torch
import torch.nn as nn
import torch.nn.init as init

from .. import kernels
from ..autograd import SegmentMseMeanFunction
from . import Trainer
from ._positional import PositionalInput, packed_pos_input
from ..training import FlatAdam, dist_info, plan_shards, step_video_total


class Transformer(PositionalInput, nn.Module):
    def __init__(self, input_size=1024, encoder_layers=6, attention_heads=8, more_residuals=False, max_length=None,
                 pos_embed="simple", epsilon=1e-5, weight_init=None, attention="dense", attention_train="dense",
                 attention_precision="fp32", attention_train_precision="fp32"):
        super().__init__()
        # attention (not in the reference, opt-in): how a no-grad call computes the multi-head attention of every layer.
        #   "dense"   heads x T x T logits per video in the workspace (csrc/transformer.hip): the default, every precision;
        #   "stream"  no logits anywhere: one fused launch per layer (csrc/attn_stream.hip), exact fp32 only -- the workspace is
        #             O(T (D + F)), so a video of 65 536 steps scores in under 8 GiB where "dense" would ask for over 100 GB.
        # attention_train (opt-in too, independent of `attention`): the same choice for a call that records a graph (training).
        #   "dense"   keeps alpha and dropout(alpha), two heads x T x T blocks per video and LAYER: the default, its bits unchanged;
        #   "stream"  keeps 8 bytes per (row, head) and layer and recomputes the weights in the backward (csrc/attn_stream_bwd.hip):
        #             exact fp32 only, head widths up to 128, the same dropout masks as "dense" for the same seed.
        # attention_precision (opt-in, attention="stream" only; governs the no-grad branch alone): the arithmetic of the attention products.
        #   "fp32"    exact (csrc/attn_stream.hip): the default, its bits unchanged;
        #   "bf16x3"  hi + lo bf16 planes, three bf16 MFMAs per product (csrc/attn_stream_split.hip): head widths % 8 == 0 up to 128;
        #             the projections stay exact fp32.  A separate argument because `precision` other than "fp32" is refused with "stream".
        # attention_train_precision (opt-in, attention_train="stream" only; governs the autograd branch alone): the same choice for training.
        #   "fp32"    exact (csrc/attn_stream.hip, csrc/attn_stream_bwd.hip): the default, its bits unchanged;
        #   "bf16x3"  the seven attention products of a training step on the bf16 MFMA (csrc/attn_stream_split.hip's training form,
        #             csrc/attn_stream_split_bwd.hip): head widths % 8 == 0 up to 128, the same masks; everything else stays exact fp32.
        if attention not in kernels.TF_ATTENTION:
            raise ValueError(f"Transformer: attention must be one of {kernels.TF_ATTENTION}, got {attention!r}")
        if attention_train not in kernels.TF_ATTENTION:
            raise ValueError(f"Transformer: attention_train must be one of {kernels.TF_ATTENTION}, got {attention_train!r}")
        if attention_precision not in kernels.TF_ATTENTION_PRECISION:
            raise ValueError(f"Transformer: attention_precision must be one of {kernels.TF_ATTENTION_PRECISION}, got {attention_precision!r}")
        if attention_precision != "fp32" and attention != "stream":
            raise ValueError(f"Transformer: attention_precision={attention_precision!r} needs attention='stream', got attention={attention!r}")
        if attention_train_precision not in kernels.TF_ATTENTION_PRECISION:
            raise ValueError(f"Transformer: attention_train_precision must be one of {kernels.TF_ATTENTION_PRECISION}, got {attention_train_precision!r}")
        if attention_train_precision != "fp32" and attention_train != "stream":
            raise ValueError(f"Transformer: attention_train_precision={attention_train_precision!r} needs attention_train='stream', "
                             f"got attention_train={attention_train!r}")
        self.attention, self.attention_train, self.attention_precision = attention, attention_train, attention_precision
        self.attention_train_precision = attention_train_precision
        self.input_size = input_size
        self.encoder_layers, self.attention_heads, self.epsilon = encoder_layers, attention_heads, epsilon
        self._init_pos_embed(max_length, pos_embed)
        self.more_residuals = more_residuals
        self.dropout = nn.Dropout(0.5)
        self.layer_norm = nn.LayerNorm(self.input_size, epsilon)
        # creation order and objects as in transformer.py:49-53 (so seeds and state_dict keys line up)
        self.transformer_encoder_layer = nn.TransformerEncoderLayer(d_model=input_size, nhead=attention_heads,
                                                                    dim_feedforward=self.input_size, dropout=0.1,
                                                                    activation="relu")
        self.transformer_encoder = nn.TransformerEncoder(encoder_layer=self.transformer_encoder_layer,
                                                         num_layers=encoder_layers, norm=self.layer_norm,
                                                         enable_nested_tensor=False)
        self.k1 = nn.Linear(self.input_size, self.input_size)
        self.k2 = nn.Linear(self.input_size, 1)
        if weight_init:
            fn = {"he": init.kaiming_uniform_, "kaiming": init.kaiming_uniform_, "xavier": init.xavier_uniform_}.get(weight_init.lower())
            if fn is not None:                                                  # transformer.py:58-70
                for i in range(self.transformer_encoder.num_layers):
                    fn(self.transformer_encoder.layers[i].linear1.weight)
                    fn(self.transformer_encoder.layers[i].linear2.weight)
                fn(self.k1.weight); fn(self.k2.weight)
        self._seed_counter = 0

    def score_packed(self, x_packed, lens):
        """x_packed: (sum(lens), D) frames of several videos back to back -> (sum(lens),) scores.  With `max_length`, frame t of every
        video gets row t of the positional table (transformer.py:82-88 at batch size 1) through an OUT-OF-PLACE add: score_packed never
        mutates x_packed (only `forward` reproduces the reference's in-place add)."""
        sb = kernels.SeqBatch.get(lens, x_packed.device)
        if self.max_length is None:
            return self._score(x_packed, sb, None, None)
        # (the split-bf16 encoder splits its layer inputs itself: the fp32 sum is all it takes)
        xp, _ = packed_pos_input(self, x_packed, sb, getattr(self, "precision", "fp32"), 0)
        return self._score(xp, sb, None, None)

    def _score(self, xp, sb, table, rows):
        """Every branch is one call of kernels.transformer_forward_packed: the library runs one layer loop under one plan, and the
        arguments below only name the path.  The no-grad branch follows attention / attention_precision: "stream" scores without the
        (T x T) logits (exact fp32; any other `precision` raises ValueError), its attention products in attention_precision.  The
        autograd branch follows attention_train / attention_train_precision alone: "dense" (default) gives the gradients it always gave,
        bit for bit; "stream" trains without the (T x T) blocks (exact fp32; any other `precision` raises), with "bf16x3" the attention
        products in bf16x3 and everything else exact fp32."""
        p = dict(self.named_parameters())
        opts = dict(layer_eps=1e-5, final_eps=self.epsilon, more_residuals=self.more_residuals,
                    precision=getattr(self, "precision", "fp32"))
        if torch.is_grad_enabled() and any(q.requires_grad for q in self.parameters()):
            from ..autograd import TransformerFunction
            if self.training:
                self._seed_counter += 1
                opts.update(layer_dropout_p=float(self.transformer_encoder.layers[0].dropout.p),
                            head_dropout_p=float(self.dropout.p),
                            seed=(torch.initial_seed() * 1000003 + self._seed_counter) & (2**63 - 1))
            names = kernels.transformer_param_names(self.encoder_layers)
            cfg = dict(n_layers=self.encoder_layers, n_heads=self.attention_heads, dff=self.input_size)
            if self.attention_train == "stream":
                if opts["precision"] not in (None, "fp32"):
                    raise ValueError(f"Transformer(attention_train='stream') trains in exact fp32: precision={opts['precision']!r} needs "
                                     "attention_train='dense' (or precision='fp32' with attention_train='stream')")
                cfg["attention"] = "stream"
                cfg["attention_train_precision"] = self.attention_train_precision
            return TransformerFunction.apply(xp, sb, cfg, opts, table, rows, names, *[p[n] for n in names])
        if self.attention == "stream":
            if opts["precision"] not in (None, "fp32"):
                raise ValueError(f"Transformer(attention='stream') scores in exact fp32: precision={opts['precision']!r} needs "
                                 "attention='dense' (or precision='fp32' with attention='stream')")
            scores, _ = kernels.transformer_forward_packed(xp, sb, p, self.encoder_layers, self.attention_heads, self.input_size,
                                                           opts, table, rows, attention="stream",
                                                           attention_precision=self.attention_precision)
            return scores
        if opts["precision"] in kernels.PLANES_OF:          # inference in a split-bf16 arithmetic: every projection on the plane GEMM
            opts["wplanes"] = self._wplanes(p, opts["precision"])
        scores, _ = kernels.transformer_forward_packed(xp, sb, p, self.encoder_layers, self.attention_heads, self.input_size,
                                                       opts, table, rows)
        return scores

    def _wplanes(self, p, precision):
        """Cached weight-plane block (kernels.transformer_wplanes) of the current weights."""
        names = kernels.transformer_param_names(self.encoder_layers)
        key = kernels.weights_key([p[n] for n in names], precision)
        return kernels.cached_block(self, "_wpl", key, lambda out: kernels.transformer_wplanes(
            {n: p[n].detach() for n in names}, self.input_size, self.input_size, self.encoder_layers, kernels.PLANES_OF[precision], out=out))


class TransformerTrainer(Trainer):
    """Mirror of the reference trainer (transformer.py:106-192): per-video MSE regression with Adam, periodic test, best-
    correlation weights; same `extra_params`.  Extensions as for VASNetTrainer: `batch_videos`, video sharding + one
    flat-bucket gradient all-reduce per step under torch.distributed.  extra_params["attention"] = "stream" scores (test, summaries)
    without the (T x T) logits (Transformer's argument of that name); extra_params["attention_train"] = "stream" trains without the
    (T x T) blocks (Transformer's attention_train); each defaults to "dense" and neither implies the other.
    extra_params["attention_precision"] = "bf16x3" (with attention "stream") scores with the attention products in the split-bf16 arithmetic;
    extra_params["attention_train_precision"] = "bf16x3" (with attention_train "stream") trains with them."""
    def _init_model(self):
        ep = self.hps.extra_params
        model = Transformer(
            encoder_layers=int(ep.get("encoder_layers", 6)),
            attention_heads=int(ep.get("attention_heads", 8)),
            more_residuals=ep.get("more_residuals", False),
            max_length=int(ep["max_pos"]) if "max_pos" in ep else None,
            pos_embed=ep.get("pos_embed", "simple"),
            epsilon=float(ep.get("epsilon", 1e-5)),
            weight_init=ep.get("weight_init", None),
            attention=ep.get("attention", "dense"),
            attention_train=ep.get("attention_train", "dense"),
            attention_precision=ep.get("attention_precision", "fp32"),
            attention_train_precision=ep.get("attention_train_precision", "fp32"),
            **({"input_size": int(ep["input_size"])} if "input_size" in ep else {}))
        model.precision = ep.get("precision", "fp32")      # "fp32" | "bf16x3" (kernels.precision_code)
        if self.hps.use_cuda:
            torch.cuda.set_device(self.hps.cuda_device)
            model.cuda()
        return model

    def train(self, fold):
        self.model.train()
        train_keys, _ = self._get_train_test_keys(fold)
        self.draw_gtscores(fold, train_keys)
        dev = self._device()
        rank, world = dist_info()
        bv = int(self.hps.extra_params.get("batch_videos", 1))
        used = set(kernels.transformer_param_names(self.model.encoder_layers)) | {"pos_embed.weight"}
        self.optimizer = FlatAdam([p for n, p in self.model.named_parameters() if n in used and p.requires_grad],
                                  lr=self.hps.lr, weight_decay=self.hps.weight_decay,
                                  comm_dtype=torch.bfloat16 if getattr(self.model, "precision", "fp32") == "bf16" else None)
        self.optimizer.broadcast()                 # identical weights on every rank: ONE collective over the flat bucket
        my_keys, sizes, steps_per_epoch = plan_shards(train_keys, lambda: [self.dataset[k]["features"].shape[0] for k in train_keys], bv)
        best = self._fold_best()
        for epoch in range(self.hps.epochs):
            losses, dist_scores = [], {}
            random.shuffle(my_keys)
            for step in range(steps_per_epoch):
                keys = my_keys[step * bv:(step + 1) * bv]
                self.optimizer.zero_grad()
                if keys:
                    x, target, lens_b, sb = self._packed_batch(keys, dev)
                    # (a model with max_pos takes this packed route too: score_packed adds the positions out of place)
                    scores = self.model.score_packed(x, lens_b)
                    n_total = len(lens_b) if world == 1 else step_video_total(sizes, bv, step)
                    loss = SegmentMseMeanFunction.apply(scores, target, sb, 1.0 / n_total)   # mean over videos of the MSE per video (transformer.py:161)
                    self._keep_scores(dist_scores, keys, scores, lens_b)
                    loss.backward(gradient=kernels.one_for(loss))
                    losses.append(loss.detach())
                self.optimizer.step(grad_scale=self.optimizer.all_reduce_grads(average=False))
            self._log_epoch(fold, epoch, Loss=float(torch.stack(losses).mean()) if losses else float("nan"))
            self._evaluate_epoch(fold, epoch, best)
        self.draw_scores(fold, dist_scores)
        return best[0], best[1], best[2]
