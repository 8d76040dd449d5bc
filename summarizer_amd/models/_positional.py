"""Positional input of the two attention scorers (VASNet, Transformer): the `max_length` / `pos_embed` constructor arguments, the
reference's in-place add in `forward` (vasnet.py:106-112, transformer.py:82-88) and the out-of-place add of a packed batch."""
import numpy as np
import torch
import torch.nn as nn

from .. import kernels


def _sinusoid_table(max_length, d):
    """vasnet.py:44-48 (vectorised; same float64 -> float32 rounding as the reference's element-wise loop)."""
    pos = np.arange(max_length, dtype=np.float64)[:, None]
    i = np.arange(0, d, 2, dtype=np.float64)[None, :]
    tab = np.zeros((max_length, d), dtype=np.float32)
    tab[:, 0::2] = np.sin(pos / (10000 ** ((2 * i) / d)))
    tab[:, 1::2] = np.cos(pos / (10000 ** ((2 * (i + 1)) / d)))
    return torch.from_numpy(tab)


class PositionalInput:
    """Mixin in front of nn.Module.  The model provides `input_size` and `_score(xp, sb, table, rows)`."""

    def _init_pos_embed(self, max_length, pos_embed):
        self.max_length = max_length
        if self.max_length:
            self.pos_embed_type = pos_embed
            if pos_embed == "simple":
                self.pos_embed = nn.Embedding(self.max_length, self.input_size)
            elif pos_embed == "attention":
                self.pos_embed = _sinusoid_table(self.max_length, self.input_size)   # plain tensor, like the reference
            else:
                self.max_length = None
        self._pos_rows_cache = {}

    def _pos_table(self, device):
        if self.pos_embed_type == "simple":
            return self.pos_embed.weight
        if self.pos_embed.device != device:
            self.pos_embed = self.pos_embed.to(device)
        return self.pos_embed

    def _pos(self, T, B, device):
        """(table, rows) for the in-place positional add over batch-major packed rows r = b*T + t."""
        if self.max_length is None:
            return None, None
        assert self.max_length >= T, "input sequence has higher length than max_length"     # vasnet.py:107
        key = (T, B, str(device))
        rows = self._pos_rows_cache.get(key)
        if rows is None:
            r = np.arange(B * T)
            idx = (r % T) if self.pos_embed_type == "simple" else (r // B)     # vasnet.py:108 vs :111 (re-view quirk)
            rows = self._pos_rows_cache[key] = torch.from_numpy(idx.astype(np.int32)).to(device)
        return self._pos_table(device), rows

    def forward(self, x):
        """x: (seq_len, batch_size, input_size) -> (seq_len, batch_size, 1)"""
        seq_len, batch_size, input_size = x.shape
        kernels._require_gpu(x, f"{type(self).__name__}.forward")
        if batch_size == 1 and x.is_contiguous():
            xp = x.view(seq_len, input_size)                                   # zero-copy; pos add lands in caller's x
        else:
            xp = x.permute(1, 0, 2).contiguous().view(batch_size * seq_len, input_size)
        table, rows = self._pos(seq_len, batch_size, x.device)
        s = self._score(xp, kernels.SeqBatch.get([seq_len] * batch_size, x.device), table, rows)
        if table is not None and xp.data_ptr() != x.data_ptr():
            with torch.no_grad():                                              # mirror the caller-visible mutation
                x.copy_(xp.view(batch_size, seq_len, input_size).permute(1, 0, 2))
        return s.view(batch_size, seq_len, 1).permute(1, 0, 2)

    def load_state_dict(self, *args, **kwargs):
        self._pos_gen = getattr(self, "_pos_gen", 0) + 1      # (packed_pos_input's cached sums)
        return super().load_state_dict(*args, **kwargs)


def packed_pos_input(model, x, sb, precision, n_planes):
    """(xp, extra options) for a packed batch of a model with `max_length` (VASNet and the Transformer scorer): xp = x + table[position]
    from sumk_pos_add_packed, after which the packed pipeline runs as for a model without positions.
    Under autograd (training, or any call that records a graph) the add is a PosAddPacked node and runs every call -- the learnable table
    changes with each optimiser step; mixed-precision training takes bf16(xp) out of the same launch (options "x16").
    Inference: n_planes > 0 (the caller's plane path will be taken) adds the KB planes of xp out of the same launch (options "xplanes");
    the fp32 sum is still produced, the plane path reads it for the residual of the output projection.  The result is kept with the tensor
    OBJECT x (kernels.pos_shadow, one entry per x) and rebuilt whenever x or the table may have changed: tensor versions, the table's
    storage address, kernels.WEIGHTS_EPOCH (optimiser steps through the C ABI), load_state_dict, another stream."""
    assert model.max_length >= max(sb.lens), "input sequence has higher length than max_length"     # vasnet.py:107 / transformer.py:83
    kernels._require_gpu(x, f"{type(model).__name__}.score_packed")
    table = model._pos_table(x.device)
    if torch.is_grad_enabled() and (model.training or any(p.requires_grad for p in model.parameters())):
        from ..autograd import PosAddPacked
        if model.training and precision == "bf16" and x.numel() % 4 == 0:
            xp, x16 = PosAddPacked.apply(x, table, sb, True)
            return xp, {"x16": x16}
        return PosAddPacked.apply(x, table, sb, False), None

    def build():
        with torch.no_grad():
            y32, _, planes = kernels.pos_add_packed(x, sb, table.detach(), want_f32=True, n_planes=n_planes)
        return y32, planes
    if torch.cuda.is_current_stream_capturing():
        y32, planes = build()
    else:
        key = (x._version, id(model), getattr(model, "_pos_gen", 0), table.data_ptr(), table._version, kernels.WEIGHTS_EPOCH[0] if table.requires_grad or isinstance(table, nn.Parameter) else -1, id(sb), int(n_planes),
               torch.cuda.current_stream(x.device).cuda_stream)
        y32, planes = kernels.pos_shadow(x, key, build)
    return y32, ({"xplanes": planes} if planes is not None else None)
