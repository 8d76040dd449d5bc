"""SumGAN-Att on MI355X -- drop-in for `summarizer/models/sumgan_att.py` (reference): the Transformer selector, the Transformer
autoencoder, Summarizer, SumGANAtt and SumGANAttTrainer.

Same constructors, defaults, forward contracts and state_dict keys as the reference; the stock `nn.TransformerEncoder` /
`nn.TransformerDecoder` objects are created in the reference's order (so seeded weights match) and kept as PARAMETER CONTAINERS --
the registered-but-unused prototype layers `transformer_encoder_layer` / `transformer_decoder_layer` included.  Every stack runs on
the HIP encoder / decoder entries (csrc/tf_decoder.hip), the selector head on the frame-head kernel, the score weighting on the
row-scaling kernel, the discriminator on `summarizer_amd.models.sumgan.GAN`.  Dropout (0.1 at every site of the stock layers) uses
the deterministic hash masks of the other Transformer path.
"""
import random

import torch
import torch.nn as nn

from .. import kernels
from ..autograd import FrameHeadFunction, RowScaleFunction, TfDecoderFunction, TfEncoderFunction
from ..training import FlatAdam, dist_info
from . import Trainer
from .sumgan import GAN


def _pack(x):
    """(seq_len, batch, D) -> batch-major packed rows (batch * seq_len, D), lens"""
    T, B, D = x.shape
    xp = x.reshape(T, D) if B == 1 else x.permute(1, 0, 2).reshape(B * T, D)
    return xp.contiguous(), [T] * B


def _unpack(rows, T, B):
    return rows.view(B, T, -1).permute(1, 0, 2)


class _Seeds:
    """Per-call dropout seed of a module in training mode (as models/transformer.py: no draw from torch's generators)."""
    def __init__(self):
        self.counter = 0

    def next(self):
        self.counter += 1
        return (torch.initial_seed() * 1000003 + self.counter) & (2**63 - 1)


def _stack_opts(module_layer, training, seeds, final_eps=1e-5):
    o = dict(layer_eps=float(module_layer.norm1.eps), final_eps=float(final_eps))
    if training:
        o.update(layer_dropout_p=float(module_layer.dropout.p), seed=seeds.next())
    return o


def _encode(encoder, xp, sb, n_heads, norm, training, seeds):
    """The encoder stack of `encoder` (nn.TransformerEncoder, used as a parameter container) over packed rows."""
    n = encoder.num_layers
    p = dict(encoder.named_parameters())
    names = kernels.tf_encoder_param_names("layers.", n)
    tensors = [p[k] for k in names]
    if norm is not None:
        names = names + ["norm.weight", "norm.bias"]
        tensors = tensors + [norm.weight, norm.bias]
    dff = encoder.layers[0].linear1.out_features
    cfg = dict(n_layers=n, n_heads=n_heads, dff=dff)
    grad = torch.is_grad_enabled() and (xp.requires_grad or any(t.requires_grad for t in tensors))
    opts = _stack_opts(encoder.layers[0], training and grad, seeds, norm.eps if norm is not None else 1e-5)
    if grad:
        return TfEncoderFunction.apply(xp, sb, cfg, opts, names, *tensors)
    return kernels.tf_encoder_forward(xp, sb, tensors, n, n_heads, dff, opts)[0]


class Transformer(nn.Module):
    def __init__(self, input_size=1024, encoder_layers=4, attention_heads=8, epsilon=1e-5):
        super().__init__()
        self.input_size = input_size
        self.encoder_layers, self.attention_heads = encoder_layers, attention_heads
        # creation order and objects as in sumgan_att.py:23-35
        self.layer_norm = torch.nn.LayerNorm(input_size, epsilon)
        self.transformer_encoder_layer = nn.TransformerEncoderLayer(d_model=input_size, nhead=attention_heads, dim_feedforward=input_size)
        self.transformer_encoder = nn.TransformerEncoder(encoder_layer=self.transformer_encoder_layer, num_layers=encoder_layers,
                                                         norm=self.layer_norm, enable_nested_tensor=False)
        self.out = nn.Sequential(nn.Linear(input_size, 1), nn.Sigmoid())
        self._seeds = _Seeds()

    def forward(self, x):
        """x: (seq_len, batch_size, input_size) -> scores (seq_len, batch_size, 1)"""
        T, B, _ = x.shape
        kernels._require_gpu(x, "SumGANAtt selector")
        xp, lens = _pack(x)
        return _unpack(self.score_packed(xp, lens), T, B)

    def score_packed(self, x_packed, lens):
        sb = kernels.SeqBatch.get(lens, x_packed.device)
        h = _encode(self.transformer_encoder, x_packed, sb, self.attention_heads, self.layer_norm, self.training, self._seeds)
        if torch.is_grad_enabled() and (h.requires_grad or self.out[0].weight.requires_grad):
            return FrameHeadFunction.apply(h, self.out[0].weight, self.out[0].bias)
        return kernels.frame_head_forward(h, self.out[0].weight, self.out[0].bias)


class AutoencoderTransformer(nn.Module):
    def __init__(self, input_size=1024, encoder_layers=4, attention_heads=8, epsilon=1e-5):
        super().__init__()
        self.input_size = input_size
        self.encoder_layers, self.attention_heads = encoder_layers, attention_heads
        # creation order and objects as in sumgan_att.py:52-68
        self.transformer_encoder_layer = nn.TransformerEncoderLayer(d_model=input_size, nhead=attention_heads, dim_feedforward=input_size)
        self.transformer_encoder = nn.TransformerEncoder(encoder_layer=self.transformer_encoder_layer, num_layers=encoder_layers,
                                                         enable_nested_tensor=False)
        self.transformer_decoder_layer = nn.TransformerDecoderLayer(d_model=input_size, nhead=attention_heads, dim_feedforward=input_size)
        self.transformer_decoder = nn.TransformerDecoder(decoder_layer=self.transformer_decoder_layer, num_layers=encoder_layers)
        self._seeds = _Seeds()

    def forward(self, x):
        """x: (seq_len, batch_size, input_size) -> x_hat (seq_len, batch_size, input_size)"""
        T, B, _ = x.shape
        kernels._require_gpu(x, "SumGANAtt autoencoder")
        xp, lens = _pack(x)
        sb = kernels.SeqBatch.get(lens, x.device)
        mem = _encode(self.transformer_encoder, xp, sb, self.attention_heads, None, self.training, self._seeds)
        return _unpack(self.decode_packed(xp, mem, sb), T, B)

    def decode_packed(self, tgt, memory, sb):
        dec = self.transformer_decoder
        n = dec.num_layers
        p = dict(dec.named_parameters())
        names = kernels.tf_decoder_param_names("layers.", n)
        tensors = [p[k] for k in names]
        dff = dec.layers[0].linear1.out_features
        grad = torch.is_grad_enabled() and (tgt.requires_grad or memory.requires_grad or any(t.requires_grad for t in tensors))
        opts = _stack_opts(dec.layers[0], self.training and grad, self._seeds)
        if grad:
            return TfDecoderFunction.apply(tgt, memory, sb, dict(n_layers=n, n_heads=self.attention_heads, dff=dff), opts, names, *tensors)
        return kernels.tf_decoder_forward(tgt, memory, sb, tensors, n, self.attention_heads, dff, opts)[0]


class Summarizer(nn.Module):
    def __init__(self, input_size=1024, s_encoder_layers=2, s_attention_heads=4, ae_encoder_layers=2, ae_attention_heads=4):
        """Summarizer: Selector (Transformer) + Autoencoder Transformer."""
        super().__init__()
        self.selector = Transformer(input_size=input_size, encoder_layers=s_encoder_layers, attention_heads=s_attention_heads)
        self.ae = AutoencoderTransformer(input_size=input_size, encoder_layers=ae_encoder_layers, attention_heads=ae_attention_heads)

    def forward(self, x, uniform=False, p=0.3):
        """x: (seq_len, batch_size, input_size) -> x_hat (seq_len, batch_size, input_size), scores (seq_len, batch_size, 1)"""
        if uniform:
            seq_len, batch_size, _ = x.size()
            scores = torch.rand((seq_len, batch_size, 1)).to(x.device)
        else:
            scores = self.selector(x)
        T, B, D = x.shape
        x_weighted = RowScaleFunction.apply(x.reshape(T * B, D), scores.reshape(T * B)).view(T, B, D)   # x * scores
        x_hat = self.ae(x_weighted)
        return x_hat, scores


class SumGANAtt(nn.Module):
    def __init__(self, input_size=1024, s_encoder_layers=2, s_attention_heads=4, ae_encoder_layers=2, ae_attention_heads=4,
                 cLSTM_hidden_size=1024, cLSTM_num_layers=2):
        """SumGAN: Summarizer + GAN"""
        super().__init__()
        self.summarizer = Summarizer(input_size=input_size, s_encoder_layers=s_encoder_layers, s_attention_heads=s_attention_heads,
                                     ae_encoder_layers=ae_encoder_layers, ae_attention_heads=ae_attention_heads)
        self.gan = GAN(input_size=input_size, hidden_size=cLSTM_hidden_size, num_layers=cLSTM_num_layers)

    def forward(self, x):
        """x: (seq_len, batch_size, input_size) -> scores (seq_len, batch_size, 1): the selector alone"""
        return self.summarizer.selector(x)

    def score_packed(self, x_packed, lens):
        return self.summarizer.selector.score_packed(x_packed, lens)


class SumGANAttTrainer(Trainer):
    """Mirror of the reference trainer (sumgan_att.py:145-410), same `extra_params`.  Autoencoder pre-training (learning rate x10),
    then per video three updates with the reference's three Adam groups: selector + encoder (||phi(x) - phi(x_hat)||_2 + BCE to the
    gtscore with `sup`), decoder (reconstruction + Wasserstein generator loss), discriminator (Wasserstein critic loss, inputs
    multiplied by Gaussian noise while epoch < epoch_noise).  As in the reference, `zero_grad` clears only the group being updated and
    the gradient-norm clip (5.0) spans every parameter -- stale gradients of the other groups included (SumGANTrainer._clip_all).
    Parameters that never receive a gradient (the unused prototype layers) are left out of the flat buckets, as torch's Adam skips
    them.  One video per step: torch.distributed is refused."""

    def _init_model(self):
        ep = self.hps.extra_params
        self.input_size = int(ep.get("input_size", 1024))
        self.s_encoder_layers = int(ep.get("s_encoder_layers", 2))
        self.s_attention_heads = int(ep.get("s_attention_heads", 4))
        self.ae_encoder_layers = int(ep.get("ae_encoder_layers", 2))
        self.ae_attention_heads = int(ep.get("ae_attention_heads", 4))
        self.cLSTM_hidden_size = int(ep.get("cLSTM_hidden_size", 256))
        self.cLSTM_num_layers = int(ep.get("cLSTM_num_layers", 2))
        self.sup = bool(ep.get("sup", True))
        self.pretrain_ae = int(ep.get("pretrain_ae", 80))
        self.epoch_noise = int(ep.get("epoch_noise", 0.2 * self.hps.epochs))
        model = SumGANAtt(input_size=self.input_size, s_encoder_layers=self.s_encoder_layers, s_attention_heads=self.s_attention_heads,
                          ae_encoder_layers=self.ae_encoder_layers, ae_attention_heads=self.ae_attention_heads,
                          cLSTM_hidden_size=self.cLSTM_hidden_size, cLSTM_num_layers=self.cLSTM_num_layers)
        self.log.debug("Generator params: {}".format(sum([_.numel() for _ in model.summarizer.parameters()])))
        self.log.debug("Discriminator params: {}".format(sum([_.numel() for _ in model.gan.parameters()])))
        return model

    # ---- losses (sumgan_att.py:172-199)
    def loss_ae(self, x, x_hat):
        return torch.norm(x - x_hat, p=2)

    def loss_recons(self, h_real, h_fake):
        return torch.norm(h_real - h_fake, p=2)

    def loss_sparsity(self, scores):
        return torch.tensor(0)

    def loss_sparsity_sup(self, scores, gtscores):
        return self.loss_BCE(scores, gtscores)

    def loss_gan_generator(self, probs_fake, probs_uniform):
        return torch.mean(-0.5 * (probs_fake + probs_uniform))

    def loss_gan_discriminator(self, probs_real, probs_fake, probs_uniform):
        return torch.mean(-probs_real + 0.5 * (probs_fake + probs_uniform))

    # ---- optimiser plumbing
    @staticmethod
    def _trained(params):
        """The parameters a group's backward reaches: not the prototype layers, which no forward uses."""
        return [p for p in params if not getattr(p, "_sumk_prototype", False)]

    def _mark_prototypes(self):
        summ = self.model.summarizer
        for mod in (summ.selector.transformer_encoder_layer, summ.ae.transformer_encoder_layer, summ.ae.transformer_decoder_layer):
            for p in mod.parameters():
                p._sumk_prototype = True

    def _update(self, opt, loss):
        opt.zero_grad()
        loss.backward()
        SumGANAttTrainer._clip_all(self._buckets)
        opt.step()

    @staticmethod
    def _clip_all(buckets, max_norm=5.0):
        from .sumgan import SumGANTrainer
        SumGANTrainer._clip_all(buckets, max_norm)

    def _video(self, key, dev):
        feats, target = self._video_on_device(key, dev, want_target=True)
        return feats.unsqueeze(1), target.view(-1, 1, 1)

    def pretrain(self, fold):
        """The autoencoder alone before the adversarial game (sumgan_att.py:201-236)."""
        train_keys, _ = self._get_train_test_keys(fold)
        dev = self._device()
        ae = self.model.summarizer.ae
        opt = FlatAdam(self._trained(ae.parameters()), lr=self.hps.lr * 10.0, weight_decay=self.hps.weight_decay)
        for epoch in range(self.pretrain_ae):
            losses = []
            random.shuffle(train_keys)
            for key in train_keys:
                x, _ = self._video(key, dev)
                x_hat = ae(x)
                loss_ae = self.loss_ae(x, x_hat)
                opt.zero_grad()
                loss_ae.backward()
                self._clip_all([opt])
                opt.step()
                losses.append(loss_ae.detach())
            if epoch % 10 == 0 or epoch == self.pretrain_ae - 1:
                self.log.info(f"Pretrain: {epoch+1:3}/{self.pretrain_ae:3}   Lae: {float(torch.stack(losses).mean()):.05f}")

    def setup_optimizers(self):
        """The three Adam groups of sumgan_att.py:246-261 as flat buckets."""
        summ, gan = self.model.summarizer, self.model.gan
        mk = lambda params: FlatAdam(self._trained(params), lr=self.hps.lr, weight_decay=self.hps.weight_decay)
        self.s_e_optimizer = mk(list(summ.selector.parameters()) + list(summ.ae.transformer_encoder.parameters())
                                + list(summ.ae.transformer_encoder_layer.parameters()))
        self.d_optimizer = mk(list(summ.ae.transformer_decoder.parameters()) + list(summ.ae.transformer_decoder_layer.parameters()))
        self.c_optimizer = mk(gan.c_lstm.parameters())
        self._buckets = [self.s_e_optimizer, self.d_optimizer, self.c_optimizer]

    def train_video(self, x, y, noisy):
        """The three updates of one video (sumgan_att.py:302-367), pass by pass as the reference writes them.  x (T,1,D), y (T,1,1)
        normalised gtscore.  Returns (Lse, Ld, Lc, D(x), D(x_hat), D(x_hat_p), scores) as device tensors."""
        summ, gan = self.model.summarizer, self.model.gan
        # -- selector and encoder
        x_hat, scores = summ(x)
        _, h_real = gan(x)
        _, h_fake = gan(x_hat)
        loss_recons = self.loss_recons(h_real, h_fake)
        loss_sparsity = self.loss_sparsity_sup(scores, y) if self.sup else self.loss_sparsity(scores)
        loss_s_e = loss_recons + loss_sparsity
        self._update(self.s_e_optimizer, loss_s_e)
        # -- decoder
        x_hat, _ = summ(x)
        x_hat_p, _ = summ(x, uniform=True)
        _, h_real = gan(x)
        probs_fake, h_fake = gan(x_hat)
        probs_uniform, _ = gan(x_hat_p)
        loss_d = self.loss_recons(h_real, h_fake) + self.loss_gan_generator(probs_fake, probs_uniform)
        self._update(self.d_optimizer, loss_d)
        # -- discriminator
        x_hat, scores = summ(x)
        x_hat_p, _ = summ(x, uniform=True)
        if noisy:
            x = torch.randn_like(x) * x
            x_hat = x_hat * torch.randn_like(x_hat)
            x_hat_p = x_hat_p * torch.randn_like(x_hat_p)
        probs_real, _ = gan(x)
        probs_fake, _ = gan(x_hat)
        probs_uniform, _ = gan(x_hat_p)
        loss_c = self.loss_gan_discriminator(probs_real, probs_fake, probs_uniform)
        self._update(self.c_optimizer, loss_c)
        return (loss_s_e.detach(), loss_d.detach(), loss_c.detach(), probs_real.mean().detach(), probs_fake.mean().detach(),
                probs_uniform.mean().detach(), scores.detach())

    def train(self, fold):
        if dist_info()[1] > 1:
            raise RuntimeError("SumGANAttTrainer trains one video per step, as the reference does: torch.distributed runs are not supported")
        self.model.train()
        self._mark_prototypes()
        train_keys, _ = self._get_train_test_keys(fold)
        self.draw_gtscores(fold, train_keys)
        self.loss_BCE = nn.BCELoss()
        if self.pretrain_ae > 0:
            self.pretrain(fold)
        dev = self._device()
        self.setup_optimizers()
        best = self._fold_best()
        tags = ("Lse", "Ld", "Lc", "D_x", "D_x_hat", "D_x_hat_p")
        dist_scores = {}
        for epoch in range(self.hps.epochs):
            log = {t: [] for t in tags}
            dist_scores = {}
            random.shuffle(train_keys)
            for key in train_keys:
                x, y = self._video(key, dev)
                *vals, scores = self.train_video(x, y, noisy=epoch < self.epoch_noise)
                for t, v in zip(tags, vals):
                    log[t].append(v)
                dist_scores[key] = scores
            means = {t: float(torch.stack(v).mean()) for t, v in log.items()}
            self.log.info(f"Epoch: {f'{epoch+1}/{self.hps.epochs}':6}   " + "  ".join(
                f"{n}: {means[t]:.05f}" for n, t in (("Lse", "Lse"), ("Ld", "Ld"), ("Lc", "Lc"), ("D(x)", "D_x"),
                                                     ("D(x_hat)", "D_x_hat"), ("D(x_hat_p)", "D_x_hat_p"))))
            for t in tags:
                self.hps.writer.add_scalar(f"{self.dataset_name}/Fold_{fold+1}/Train/{t}", means[t], epoch)
            self._evaluate_epoch(fold, epoch, best)
        self.draw_scores(fold, dist_scores)
        return best[0], best[1], best[2]
