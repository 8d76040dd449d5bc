"""Stock-PyTorch (CPU, fp32) functional port of the reference scorers.  TEST INFRASTRUCTURE ONLY.
The SumGAN recurrences (lstm_stack_ref, dlstm_ref) and make_gru also run in float64: the high-precision oracles of
tests/test_gpu_sumgan_full.py; transformer_ref likewise for tests/test_gpu_transformer_f64.py, tf_encoder_stack_ref / tf_decoder_stack_ref for
tests/test_gpu_sumgan_att_f64.py, bilstm_stack_ref for
tests/test_gpu_lstm_f64.py (float64 reference and, in fp32 with the kernels' gate formulas, its yardstick), bigru_stack_ref the same
for tests/test_gpu_gru_f64.py, lstm_stack_ref / dlstm_ref (gate_math, matmul) the same for tests/test_gpu_sumgan_lstm_f64.py.

This is (1) a second, autograd-capable checker for the HIP path (forward AND gradients), and
(2) the `cpu_baseline` ("kind": "port") that bench.py times on the GPU node's host cores: it issues the
same ATen op sequence as the reference modules (Linear / bmm / softmax / layer_norm / nn.LSTM), one video
per call, exactly like Trainer.test (summarizer/models/__init__.py:45-54).
Pinned against the real reference by tests/golden/*.npz (see tests/test_oracle.py).
"""
import math
import torch
import torch.nn.functional as F


def _r16(t):
    """fp32 -> bf16 (round to nearest even, what v_cvt_pk_bf16_f32 does) -> back to the dtype of t.  A float64 t goes through fp32 first:
    the kernels round an fp32 value, so the float64 emulation (tests/vasnet_bf16_common.py) rounds at the same two steps."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class _Linear16(torch.autograd.Function):
    """y = x W^T with BOTH operands rounded to bf16 and accumulation in the dtype of x (fp32: what the kernels do; float64: the
    high-precision form of the same arithmetic) -- and the same in the backward: dx = bf16(dy) bf16(W), dW = bf16(dy)^T bf16(x).  This
    is the arithmetic of the mixed-precision training step (csrc/gemm_b16.hip: every GEMM reads bf16 shadows of its operands, gradients
    included), restated with stock matmuls (a product of two bf16 values is exact in fp32).  round_x / round_w = False: that operand is
    taken as it is (a caller that knows it to be bf16-representable)."""

    @staticmethod
    def forward(ctx, x, w, round_x=True, round_w=True):
        xr, wr = _r16(x) if round_x else x, _r16(w) if round_w else w
        ctx.save_for_backward(xr, wr)
        return xr @ wr.t()

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = _r16(dy)
        return dyr @ wr, dyr.reshape(-1, dyr.shape[-1]).t() @ xr.reshape(-1, xr.shape[-1]), None, None


class _Bmm16(torch.autograd.Function):
    """C = A B per batch entry, operands rounded to bf16 in the forward and in both backward products."""

    @staticmethod
    def forward(ctx, a, b):
        ar, br = _r16(a), _r16(b)
        ctx.save_for_backward(ar, br)
        return torch.bmm(ar, br)

    @staticmethod
    def backward(ctx, dy):
        ar, br = ctx.saved_tensors
        dyr = _r16(dy)
        return torch.bmm(dyr, br.transpose(1, 2)), torch.bmm(ar.transpose(1, 2), dyr)


def vasnet_scores(x, p, ignore_self=False, aperture=None, scale=None, eps=1e-6, pos_table=None,
                  pos_kind="simple", drop_masks=None, return_logits=False, bf16_products=False, round_leaves=True, key_mask=None):
    """x: (T,B,D) -> (T,B,1).  Op order of vasnet.py:99-147.

    drop_masks: optional (m_alpha (B,T,T), m_y (B,T,D), m_z (B,T,D)) of already-scaled keep masks
    (0 or 1/(1-p)) so training-mode dropout can be checked deterministically.
    return_logits: also return the pre-sigmoid outputs of k2 (vasnet.py:144).
    bf16_products: emulate the mixed-precision training arithmetic (see _Linear16) instead of fp32 products; everything but the
    roundings of the product operands runs in the dtype of x and p (float64: the reference of tests/vasnet_bf16_common.py).
    round_leaves=False (with bf16_products): x and the weight matrices are NOT rounded -- for inputs that are bf16 values already.
    key_mask: optional (B,T,T) bool, True = this (query, key) pair is masked as well (the seeded faults of
    tests/test_vasnet_bf16_host.py).
    """
    T, B, D = x.shape
    xb = x.permute(1, 0, 2)
    if pos_table is not None:
        bi = torch.arange(B).unsqueeze(1); ti = torch.arange(T).unsqueeze(0)
        rows = ti.expand(B, T) if pos_kind == "simple" else (bi * T + ti) // B     # vasnet.py:108-111 (see vasnet_np.pos_rows)
        xb = xb + pos_table[rows]
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    # bf16_products: the emulated mixed-precision arithmetic (precision="bf16"): every matrix product on bf16-rounded operands with
    # fp32 accumulation, forward and backward; softmax / LayerNorm / residual / head stay fp32 as in csrc/vasnet.hip
    rl = bool(round_leaves)
    lin = (lambda a, w_, b_=None, ra=True: _Linear16.apply(a, w_, ra, rl) + (b_ if b_ is not None else 0.0)) if bf16_products else \
        (lambda a, w_, b_=None, ra=True: F.linear(a, w_, b_))
    bmm = _Bmm16.apply if bf16_products else torch.bmm
    K = lin(xb, p["K.weight"], None, rl); Q = lin(xb, p["Q.weight"], None, rl); V = lin(xb, p["V.weight"], None, rl)
    e = bmm(Q, K.transpose(1, 2)) * sc
    if key_mask is not None:
        e = e.masked_fill(key_mask, float("-inf"))
    if ignore_self:
        e = e.masked_fill(torch.eye(T, dtype=torch.bool, device=e.device).unsqueeze(0), float("-inf"))
    if aperture is not None:
        scope = torch.tril(e, diagonal=aperture) * torch.triu(e, diagonal=-aperture)
        e = e.masked_fill(scope == 0, float("-inf"))
    alpha = torch.softmax(e, dim=2)
    if drop_masks is not None:
        alpha = alpha * drop_masks[0]
    c = lin(bmm(alpha, V), p["attention_head_projection.weight"])
    y = c + xb
    if drop_masks is not None:
        y = y * drop_masks[1]
    y = F.layer_norm(y, (D,), p["layer_norm.weight"], p["layer_norm.bias"], eps)
    z = torch.relu(lin(y, p["k1.weight"], p["k1.bias"]))
    if drop_masks is not None:
        z = z * drop_masks[2]
    z = F.layer_norm(z, (D,), p["layer_norm.weight"], p["layer_norm.bias"], eps)
    u = F.linear(z, p["k2.weight"], p["k2.bias"])
    s = torch.sigmoid(u)
    if return_logits:            # (scores, pre-sigmoid k2 outputs): where scores saturate, the logits still tell two paths apart
        return s.permute(1, 0, 2), u.permute(1, 0, 2)
    return s.permute(1, 0, 2)


def make_lstm(p, prefix, input_size, hidden_size, num_layers):
    """Builds a stock nn.LSTM carrying the given weights (dsn.py:23-27 / sumgan.py:27-32)."""
    m = torch.nn.LSTM(input_size, hidden_size, num_layers=num_layers, bidirectional=True)
    sd = {k[len(prefix):]: torch.as_tensor(v) for k, v in p.items() if k.startswith(prefix)}
    m.load_state_dict(sd)
    return m


def bilstm_scores(x, p, prefix, head_w, head_b, input_size, hidden_size, num_layers, lstm=None):
    lstm = lstm if lstm is not None else make_lstm(p, prefix, input_size, hidden_size, num_layers)
    h, _ = lstm(x)
    return torch.sigmoid(F.linear(h, p[head_w], p[head_b]))


class TransformerPort(torch.nn.Module):
    """Stock-PyTorch restatement of the reference Transformer scorer (transformer.py:19-103) with every dropout at 0:
    learnable positional table added in place, nn.TransformerEncoder (post-norm, FF = D) whose final norm is the SAME
    LayerNorm that follows k1, then k1 / ReLU / LayerNorm / k2 / sigmoid.  Autograd-capable checker for the HIP path."""

    def __init__(self, D, n_layers, n_heads, max_length=None, eps=1e-5, more_residuals=False):
        super().__init__()
        nn = torch.nn
        self.pos_embed = nn.Embedding(max_length, D) if max_length else None
        self.layer_norm = nn.LayerNorm(D, eps)
        layer = nn.TransformerEncoderLayer(d_model=D, nhead=n_heads, dim_feedforward=D, dropout=0.0, activation="relu")
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=n_layers, norm=self.layer_norm, enable_nested_tensor=False)
        self.k1, self.k2 = nn.Linear(D, D), nn.Linear(D, 1)
        self.more_residuals = more_residuals

    def forward(self, x):
        T, B, D = x.shape
        if self.pos_embed is not None:
            x = x + self.pos_embed(torch.arange(T)).unsqueeze(1)          # 'simple' table: row t for every batch entry
        e = self.transformer_encoder(x)
        if self.more_residuals:
            e = e + x
        return torch.sigmoid(self.k2(self.layer_norm(torch.relu(self.k1(e)))))


def _relu_logged(a, w, b, relu_log):
    """relu(a W^T + b); relu_log (optional list) gets (pre-activation, sum_k |w_k a_k| + |b|), see transformer_ref."""
    pre = F.linear(a, w, b)
    if relu_log is not None:
        relu_log.append((pre.detach(), F.linear(a.detach().abs(), w.detach().abs(), b.detach().abs())))
    return torch.relu(pre)


def _tf_attend(q, k, v, lens, n_heads, amasks):
    """Multi-head attention per video over packed rows: q, k, v (R, D) -> context (R, D).  amasks: [(heads, T_i, T_i)] or None."""
    D = q.shape[1]
    dh = D // n_heads
    ctx, r0 = [], 0
    for i, T in enumerate(lens):
        qh, kh, vh = (t[r0:r0 + T].reshape(T, n_heads, dh).transpose(0, 1) for t in (q, k, v))
        a = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(dh), dim=-1)               # (heads, T, T)
        if amasks is not None:
            a = a * amasks[i]
        ctx.append((a @ vh).transpose(0, 1).reshape(T, D))
        r0 += T
    return torch.cat(ctx)


def _tf_self_attn(h, g, pre, lens, n_heads, amasks, omask):
    """dropout1(out_proj(MHA(h, h, h))) of a stock post-norm layer (keys pre + "self_attn.*"), without residual and norm."""
    D = h.shape[1]
    qkv = F.linear(h, g(pre + "self_attn.in_proj_weight"), g(pre + "self_attn.in_proj_bias"))
    ctx = _tf_attend(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], lens, n_heads, amasks)
    o = F.linear(ctx, g(pre + "self_attn.out_proj.weight"), g(pre + "self_attn.out_proj.bias"))
    return o if omask is None else o * omask


def _tf_cross_attn(h, mem, g, pre, lens, n_heads, amasks, omask):
    """dropout2(out_proj(MHA(h, mem, mem))) of a stock decoder layer (keys pre + "multihead_attn.*"): Q from rows [0, D) of
    in_proj, K / V from rows [D, 3D) applied to the memory."""
    D = h.shape[1]
    w, b = g(pre + "multihead_attn.in_proj_weight"), g(pre + "multihead_attn.in_proj_bias")
    q = F.linear(h, w[0:D], b[0:D])
    kv = F.linear(mem, w[D:3 * D], b[D:3 * D])
    ctx = _tf_attend(q, kv[:, 0:D], kv[:, D:2 * D], lens, n_heads, amasks)
    o = F.linear(ctx, g(pre + "multihead_attn.out_proj.weight"), g(pre + "multihead_attn.out_proj.bias"))
    return o if omask is None else o * omask


def _tf_ff(h, g, pre, m1, m2, relu_log):
    """dropout_b(linear2(dropout_a(relu(linear1(h))))) of a stock layer; F is linear1's row count."""
    f = _relu_logged(h, g(pre + "linear1.weight"), g(pre + "linear1.bias"), relu_log)
    if m1 is not None:
        f = f * m1
    f = F.linear(f, g(pre + "linear2.weight"), g(pre + "linear2.bias"))
    return f if m2 is None else f * m2


def _tf_encoder_layers(h, g, prefix, lens, n_layers, n_heads, layer_eps, masks, relu_log):
    """n stock post-norm nn.TransformerEncoderLayer over packed rows h (R, D); keys prefix + f"{l}." + the layer's own."""
    D = h.shape[1]
    for l in range(n_layers):
        pre = f"{prefix}{l}."
        mk = (lambda site: masks[site][l]) if masks is not None else (lambda site: None)
        o = _tf_self_attn(h, g, pre, lens, n_heads, mk("attn"), mk("out"))
        h = F.layer_norm(h + o, (D,), g(pre + "norm1.weight"), g(pre + "norm1.bias"), layer_eps)
        f = _tf_ff(h, g, pre, mk("ff1"), mk("ff2"), relu_log)
        h = F.layer_norm(h + f, (D,), g(pre + "norm2.weight"), g(pre + "norm2.bias"), layer_eps)
    return h


def transformer_ref(xs, params, n_layers, n_heads, layer_eps=1e-5, final_eps=1e-5, more_residuals=False, pos=None, masks=None,
                    relu_log=None):
    """Functional restatement of the reference Transformer scorer (transformer.py:74-103 over stock post-norm
    nn.TransformerEncoderLayer, FF = D) for a ragged list of videos, in the dtype of the inputs, with plain torch ops.
    The high-precision oracle of tests/test_gpu_transformer_f64.py (run there in float64); differentiable in xs, params, pos.

    xs: [(T_i, D)]; params: the model's state_dict keys (kernels.transformer_param_names).
    pos: optional (table (n, D), rows (sum T_i,) int): row r of the packed batch adds table[rows[r]] (Transformer._pos).
    masks: optional already-scaled keep-masks (0 or 1/(1-p)) as built by recipes.transformer_drop_masks:
      {"attn": [[(heads, T_i, T_i) per video] per layer], "out" / "ff1" / "ff2": [(R, D) / (R, F) / (R, D) per layer],
       "head": (R, D)} -- rows are PACKED rows, as the kernels index them.
    relu_log: optional list; for every ReLU (linear1 of each layer, then k1) appends (pre-activation, sum_k |w_k a_k| + |b|) -- the scale of
    the rounding error an fp32 evaluation of that pre-activation carries (how close to the kink a unit may lie before it can flip).
    Returns (scores, logits): packed (R,) each."""
    g = lambda k: params[k]
    lens = [int(x.shape[0]) for x in xs]
    x = torch.cat(list(xs))
    if pos is not None:
        x = x + pos[0][torch.as_tensor(pos[1], device=x.device).long()]
    D = x.shape[1]
    h = _tf_encoder_layers(x, g, "transformer_encoder.layers.", lens, n_layers, n_heads, layer_eps, masks, relu_log)
    h = F.layer_norm(h, (D,), g("layer_norm.weight"), g("layer_norm.bias"), final_eps)       # encoder's final norm = the shared LN
    if more_residuals:
        h = h + x
    z = _relu_logged(h, g("k1.weight"), g("k1.bias"), relu_log)
    if masks is not None:
        z = z * masks["head"]
    z = F.layer_norm(z, (D,), g("layer_norm.weight"), g("layer_norm.bias"), final_eps)        # the same LN again
    u = F.linear(z, g("k2.weight"), g("k2.bias"))[:, 0]
    return torch.sigmoid(u), u


def tf_encoder_stack_ref(xs, params, prefix, n_layers, n_heads, layer_eps=1e-5, final_norm=None, final_eps=1e-5, masks=None,
                         relu_log=None):
    """SumGAN-Att's encoder stack (sumgan_att.py:20-80: n stock post-norm nn.TransformerEncoderLayer, then an optional final
    LayerNorm) for a ragged list of videos, in the dtype of the inputs, with plain torch ops: the float64 oracle (and, in fp32, the
    yardstick) of tests/test_gpu_sumgan_att_f64.py.  Differentiable in xs and params.

    xs: [(T_i, D)]; params: keys prefix + f"{l}." + nn.TransformerEncoderLayer's own (kernels.tf_encoder_param_names); the
    feed-forward width F is linear1's row count.  final_norm: key prefix of the final LayerNorm (e.g. "norm."), or None.
    masks: optional already-scaled keep-masks as built by recipes.tf_stack_drop_masks(decoder=False), in transformer_ref's layout
    (packed rows); relu_log: as transformer_ref.  Returns the packed hidden states (R, D)."""
    g = lambda k: params[k]
    lens = [int(x.shape[0]) for x in xs]
    h = torch.cat(list(xs))
    D = h.shape[1]
    h = _tf_encoder_layers(h, g, prefix, lens, n_layers, n_heads, layer_eps, masks, relu_log)
    if final_norm is not None:
        h = F.layer_norm(h, (D,), g(final_norm + "weight"), g(final_norm + "bias"), final_eps)
    return h


def tf_decoder_stack_ref(tgts, mems, params, prefix, n_layers, n_heads, layer_eps=1e-5, masks=None, relu_log=None):
    """SumGAN-Att's decoder stack (n stock post-norm nn.TransformerDecoderLayer, ReLU, no attention masks: norm1(t + SA(t)),
    norm2(. + CA(., memory)), norm3(. + FF(.))) for a ragged list of videos, in the dtype of the inputs, with plain torch ops.
    Differentiable in tgts, mems and params.

    tgts, mems: [(T_i, D)], video i of the target attends to video i of the memory; params: keys prefix + f"{l}." +
    nn.TransformerDecoderLayer's own (kernels.tf_decoder_param_names).  masks: optional already-scaled keep-masks as built by
    recipes.tf_stack_drop_masks(decoder=True): transformer_ref's per-layer entries plus "cattn" [[(heads, T_i, T_i) per video] per
    layer] on the cross-attention weights and "cout" [(R, D) per layer] on its out-projection (dropout2).  relu_log: as
    transformer_ref.  Returns the packed outputs (R, D)."""
    g = lambda k: params[k]
    lens = [int(x.shape[0]) for x in tgts]
    assert lens == [int(x.shape[0]) for x in mems]
    h, mem = torch.cat(list(tgts)), torch.cat(list(mems))
    D = h.shape[1]
    for l in range(n_layers):
        pre = f"{prefix}{l}."
        mk = (lambda site: masks[site][l]) if masks is not None else (lambda site: None)
        h = F.layer_norm(h + _tf_self_attn(h, g, pre, lens, n_heads, mk("attn"), mk("out")), (D,), g(pre + "norm1.weight"),
                         g(pre + "norm1.bias"), layer_eps)
        h = F.layer_norm(h + _tf_cross_attn(h, mem, g, pre, lens, n_heads, mk("cattn"), mk("cout")), (D,), g(pre + "norm2.weight"),
                         g(pre + "norm2.bias"), layer_eps)
        h = F.layer_norm(h + _tf_ff(h, g, pre, mk("ff1"), mk("ff2"), relu_log), (D,), g(pre + "norm3.weight"),
                         g(pre + "norm3.bias"), layer_eps)
    return h


def make_gru(p, prefix, input_size, hidden_size, num_layers, dtype=torch.float32):
    """Stock nn.GRU carrying the given weights (the reference's optional DSN(cell="gru"), dsn.py:28-33), in `dtype`
    (torch.float64 for a high-precision reference: the weights are converted, so feed it inputs of the same dtype)."""
    m = torch.nn.GRU(input_size, hidden_size, num_layers=num_layers, bidirectional=True).to(dtype)
    m.load_state_dict({k[len(prefix):]: torch.as_tensor(v) for k, v in p.items() if k.startswith(prefix)})
    return m


def _lstm_cell(gx, h, c, w_hh, b_hh, sig=torch.sigmoid, tanh=torch.tanh, mm=None):
    """One nn.LSTM step: gx = x W_ih^T + b_ih (precomputed); gate order i, f, g, o as in torch.  mm: the matmul hook of
    lstm_stack_ref / dlstm_ref -- gx then carries BOTH biases already (as the kernels' pre-activations do) and b_hh is not added."""
    pre = gx + F.linear(h, w_hh, b_hh) if mm is None else gx + mm(h, w_hh, "hh")
    i, f, g, o = pre.chunk(4, dim=-1)
    c = sig(f) * c + sig(i) * tanh(g)
    return sig(o) * tanh(c), c


def _num_layers(params):
    return sum(1 for k in params if k.startswith("weight_ih_l"))


def lstm_stack_ref(x_list, params, h0=None, c0=None, gate_math="exact", matmul=None, layer_outs=None):
    """Forward-running nn.LSTM(num_layers=L, bidirectional=False) over a ragged list of videos, in the dtype of the inputs.
    x_list: [(T_i, In)]; params: nn.LSTM state_dict names (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, ...);
    h0 / c0: (L, B, H) or None (zeros).  Returns ([out_i (T_i, H)] of the top layer, (h_n, c_n) (L, B, H)): the state after
    each video's OWN last frame.  Videos run side by side, time-major; a video that has ended keeps its state.  Everything
    is differentiable (inputs, parameters, initial state).
    gate_math: a key of GATE_MATH.  matmul: optional hook (a (n, K), w (N, K), site) -> a @ w.T with site "ih" (input projection) or
    "hh" (recurrent product), as in bilstm_stack_ref (Linear3, LinearDw3, LinearChainDx); with a hook the sums run in the kernels' order
    (csrc/lstm.hip: the projection's epilogue adds b_ih and b_hh, a step adds the recurrent product to that).  The defaults keep the
    plain F.linear form bit for bit.  layer_outs: optional list that receives [h_i (T_i, H) per video] of every layer."""
    sig, tanh = GATE_MATH[gate_math]
    L, B = _num_layers(params), len(x_list)
    H = params["weight_hh_l0"].shape[1]
    lens = [int(x.shape[0]) for x in x_list]
    T = max(lens)
    ref = x_list[0]
    act = torch.tensor([[t < n for n in lens] for t in range(T)]).unsqueeze(-1)      # (T, B, 1)
    seq = torch.nn.utils.rnn.pad_sequence(list(x_list))                              # (T, B, In), zero padded
    hn, cn = [], []
    for l in range(L):
        if matmul is None:
            gx = F.linear(seq, params[f"weight_ih_l{l}"], params[f"bias_ih_l{l}"])       # input projection, all frames at once
        else:
            gx = (matmul(seq.reshape(T * B, -1), params[f"weight_ih_l{l}"], "ih") + params[f"bias_ih_l{l}"]
                  + params[f"bias_hh_l{l}"]).reshape(T, B, 4 * H)
        h = h0[l] if h0 is not None else ref.new_zeros(B, H)
        c = c0[l] if c0 is not None else ref.new_zeros(B, H)
        outs = []
        for t in range(T):
            hs, cs = _lstm_cell(gx[t], h, c, params[f"weight_hh_l{l}"], params[f"bias_hh_l{l}"], sig, tanh, matmul)
            h, c = torch.where(act[t], hs, h), torch.where(act[t], cs, c)
            outs.append(h)
        seq = torch.stack(outs)
        hn.append(h); cn.append(c)
        if layer_outs is not None:
            layer_outs.append([seq[:n, b] for b, n in enumerate(lens)])
    return [seq[:n, b] for b, n in enumerate(lens)], (torch.stack(hn), torch.stack(cn))


GATE_MATH = {
    # "exact": torch's own sigmoid / tanh.  "rcp_form": the formulas of the recurrence kernels (csrc/persist_common.h: fast_sigmoid,
    # fast_tanh) in plain torch ops, so that autograd differentiates the same formula the kernels evaluate.
    # "rcp_sigmoid": the launch-per-step kernels of csrc/lstm.hip (sigmoidf_ = 1 / (1 + expf(-v)) next to the library's tanhf).
    "exact": (torch.sigmoid, torch.tanh),
    "rcp_form": (lambda v: 1.0 / (1.0 + torch.exp(-v)), lambda v: 1.0 - 2.0 / (1.0 + torch.exp(2.0 * v))),
    "rcp_sigmoid": (lambda v: 1.0 / (1.0 + torch.exp(-v)), torch.tanh),
}


def split_bf16(x):
    """x ~= hi + lo, both bf16 values held in the dtype of x (the two operand planes of the bf16x3 arithmetic)."""
    hi = x.to(torch.bfloat16).to(x.dtype)
    return hi, (x - hi).to(torch.bfloat16).to(x.dtype)


def mm3(a, b):
    """a @ b as the bf16x3 MFMA path takes it: hi.hi + hi.lo + lo.hi on two-plane operands (lo.lo dropped), products exact and summed
    in the dtype of the operands (tests/probes/bf16x3_emulation.py)."""
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
    return ah @ bh + (ah @ bl + al @ bh)


class Linear3(torch.autograd.Function):
    """y = x W^T (2-D x) in bf16x3, with the backward products the library runs for a layer of that precision: dW = dy^T x in bf16x3,
    dx = dy W in bf16x3 -- or exactly (exact_dx: the BPTT multiplies dG by W_hh in fp32 whatever the layer's precision)."""

    @staticmethod
    def forward(ctx, x, w, exact_dx):
        ctx.save_for_backward(x, w)
        ctx.exact_dx = exact_dx
        return mm3(x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return (dy @ w if ctx.exact_dx else mm3(dy, w)), mm3(dy.t(), x), None


def mm_chain(a, b):
    """a (M, K) @ b (K, N) summed as ONE accumulator per output element walks k in the exact-fp32 MFMA GEMM (csrc/gemm_regstage.h:
    v_mfma_f32_32x32x2_f32 adds two k into the accumulator per issue; within each block of 8 k the issues pair k with k + 4), in the
    dtype of the operands.  A BLAS sums K terms in blocks and lanes, so its rounding error grows far slower with K than the
    chain's: for a long K this, not a BLAS product, is what the fp32 yardstick of such a GEMM has to be."""
    K = a.shape[1]
    acc = a.new_zeros(a.shape[0], b.shape[1])
    for k0 in range(0, K - K % 8, 8):
        for j in range(4):
            acc = torch.addmm(acc, a[:, [k0 + j, k0 + 4 + j]], b[[k0 + j, k0 + 4 + j]])
    for k in range(K - K % 8, K):
        acc = torch.addmm(acc, a[:, k:k + 1], b[k:k + 1])
    return acc


class LinearChainDx(torch.autograd.Function):
    """y = x W^T (2-D x) whose backward takes dx = dy W with mm_chain: the dX GEMM of sumk_bilstm_layer_backward sums K = 4H gate
    columns per direction in one accumulator chain (up to 4096 terms at H = 1024); the weight gradient stays a plain product (the
    library sums it as split-K: many short chains)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return x @ w.t()

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return mm_chain(dy, w), dy.t() @ x


def bilstm_stack_ref(x_list, params, gate_math="exact", matmul=None):
    """Stacked nn.LSTM(num_layers=L, bidirectional=True) over a ragged list of videos, written out step by step with plain torch
    ops in the dtype of the inputs (float64: the reference of tests/test_gpu_lstm_f64.py; float32: its yardstick).
    x_list: [(T_i, In)]; params: nn.LSTM state_dict names (weight_ih_l0, weight_ih_l0_reverse, ...).
    gate_math: a key of GATE_MATH.  matmul: optional hook (a (n, K), w (N, K), site) -> a @ w.T with site "ih" (input projection) or
    "hh" (recurrent product), e.g. Linear3 for the layers the library runs in bf16x3; None: a @ w.T in the dtype.
    The videos run side by side in descending order of length, each direction over its own frames only (the reverse direction
    starts at a video's LAST frame).  As in the kernels, the input projection of all frames comes first and carries both biases.
    Returns [[h_i (T_i, 2H) = [h_fwd || h_rev] per video] per layer]; differentiable in inputs and parameters."""
    sig, tanh = GATE_MATH[gate_math]
    mm = matmul if matmul is not None else (lambda a, w, site: a @ w.t())
    L = sum(1 for k in params if k.startswith("weight_ih_l") and not k.endswith("_reverse"))
    H = params["weight_hh_l0"].shape[1]
    lens = [int(x.shape[0]) for x in x_list]
    order = sorted(range(len(lens)), key=lambda i: -lens[i])
    n_act = [sum(1 for n in lens if n > t) for t in range(max(lens))]                # videos still running at step t: a prefix of `order`
    layers, cur = [], list(x_list)
    for l in range(L):
        halves = []
        for suf in ("", "_reverse"):
            w_ih, w_hh = params[f"weight_ih_l{l}{suf}"], params[f"weight_hh_l{l}{suf}"]
            bias = params[f"bias_ih_l{l}{suf}"] + params[f"bias_hh_l{l}{suf}"]
            own = [torch.flip(cur[i], (0,)) if suf else cur[i] for i in order]       # each video in this direction's step order
            seq = torch.nn.utils.rnn.pad_sequence(own)                               # (T_max, B, In)
            gx = (mm(seq.reshape(-1, seq.shape[-1]), w_ih, "ih") + bias).reshape(seq.shape[0], seq.shape[1], 4 * H)
            h = c = seq.new_zeros(len(lens), H)
            outs = []
            for t, nb in enumerate(n_act):
                i, f, g, o = (gx[t, :nb] + mm(h[:nb], w_hh, "hh")).chunk(4, dim=-1)
                c = sig(f) * c[:nb] + sig(i) * tanh(g)
                h = sig(o) * tanh(c)
                outs.append(torch.cat([h, h.new_zeros(len(lens) - nb, H)]) if nb < len(lens) else h)
            out = torch.stack(outs)                                                  # (T_max, B, H), rows in `order`
            per = [None] * len(lens)
            for r, i in enumerate(order):
                per[i] = torch.flip(out[:lens[i], r], (0,)) if suf else out[:lens[i], r]
            halves.append(per)
        cur = [torch.cat([a, b], dim=1) for a, b in zip(*halves)]
        layers.append(cur)
    return layers


class LinearDw3(torch.autograd.Function):
    """y = x W^T (2-D x) taken exactly, forward and dx = dy W, whose WEIGHT gradient alone is dW = dy^T x in bf16x3: the recurrent
    product of the persistent GRU layer in that precision (csrc/gru_persist.hip: the recurrence and the BPTT's dGh . W_hh multiply in
    fp32 inside the kernels; the split-K launches of dW_hh take the layer's precision)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return x @ w.t()

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return dy @ w, mm3(dy.t(), x)


def _gru_cell(gx, hw, b_hh, h, sig, tanh):
    """One nn.GRU step: gx = x W_ih^T + b_ih (precomputed), hw = h W_hh^T; gate order r, z, n as in torch, b_hn inside r * (...).
    The sums in the kernels' order: gx + (hw + b_hh)."""
    xr, xz, xn = gx.chunk(3, dim=-1)
    hr, hz, hn = (hw + b_hh).chunk(3, dim=-1)
    r, z = sig(xr + hr), sig(xz + hz)
    n = tanh(xn + r * hn)
    return (1.0 - z) * n + z * h


def bigru_stack_ref(x_list, params, gate_math="exact", matmul=None):
    """Stacked nn.GRU(num_layers=L, bidirectional=True) over a ragged list of videos, written out step by step with plain torch ops
    in the dtype of the inputs (float64: the reference of tests/test_gpu_gru_f64.py; float32: its yardstick) -- bilstm_stack_ref's
    twin.  x_list: [(T_i, In)]; params: nn.GRU state_dict names (weight_ih_l0, weight_ih_l0_reverse, ...).
    gate_math: a key of GATE_MATH.  matmul: optional hook (a (n, K), w (N, K), site) -> a @ w.T with site "ih" (input projection) or
    "hh" (recurrent product); None: a @ w.T in the dtype.
    The videos run side by side in descending order of length, each direction over its own frames only (the reverse direction
    starts at a video's LAST frame).  As in the kernels, the input projection of all frames comes first and carries b_ih; b_hh joins
    the recurrent product in every step (r multiplies b_hn).
    Returns [[h_i (T_i, 2H) = [h_fwd || h_rev] per video] per layer]; differentiable in inputs and parameters."""
    sig, tanh = GATE_MATH[gate_math]
    mm = matmul if matmul is not None else (lambda a, w, site: a @ w.t())
    L = sum(1 for k in params if k.startswith("weight_ih_l") and not k.endswith("_reverse"))
    H = params["weight_hh_l0"].shape[1]
    lens = [int(x.shape[0]) for x in x_list]
    order = sorted(range(len(lens)), key=lambda i: -lens[i])
    n_act = [sum(1 for n in lens if n > t) for t in range(max(lens))]                # videos still running at step t: a prefix of `order`
    layers, cur = [], list(x_list)
    for l in range(L):
        halves = []
        for suf in ("", "_reverse"):
            w_ih, w_hh = params[f"weight_ih_l{l}{suf}"], params[f"weight_hh_l{l}{suf}"]
            b_ih, b_hh = params[f"bias_ih_l{l}{suf}"], params[f"bias_hh_l{l}{suf}"]
            own = [torch.flip(cur[i], (0,)) if suf else cur[i] for i in order]       # each video in this direction's step order
            seq = torch.nn.utils.rnn.pad_sequence(own)                               # (T_max, B, In)
            gx = (mm(seq.reshape(-1, seq.shape[-1]), w_ih, "ih") + b_ih).reshape(seq.shape[0], seq.shape[1], 3 * H)
            h = seq.new_zeros(len(lens), H)
            outs = []
            for t, nb in enumerate(n_act):
                h = _gru_cell(gx[t, :nb], mm(h[:nb], w_hh, "hh"), b_hh, h[:nb], sig, tanh)
                outs.append(torch.cat([h, h.new_zeros(len(lens) - nb, H)]) if nb < len(lens) else h)
            out = torch.stack(outs)                                                  # (T_max, B, H), rows in `order`
            per = [None] * len(lens)
            for r, i in enumerate(order):
                per[i] = torch.flip(out[:lens[i], r], (0,)) if suf else out[:lens[i], r]
            halves.append(per)
        cur = [torch.cat([a, b], dim=1) for a, b in zip(*halves)]
        layers.append(cur)
    return layers


def dlstm_ref(params, recons, T, h0, c0, gate_math="exact", matmul=None):
    """SumGAN's step-wise decoder (dLSTM, sumgan.py:74-115) in the dtype of h0: an nn.LSTM stack run one step at a time
    whose input at step t is its own top-layer output of step t-1 (zeros at t = 0), then recons = (weight, bias) on every
    output, then time reversed.  T: one length for every video, or a list of per-video lengths (each video decodes its own
    steps; the others do not see them).  h0 / c0: (L, B, H).  Returns [x_hat_i (T_i, out)]; with recons=None, the top
    layer's outputs [(T_i, H)] in time order (neither projected nor reversed: what the decoder kernels return).
    gate_math / matmul: as lstm_stack_ref; with a hook both biases join the input product before the recurrent product is added
    (the decoder kernels add b_ih + b_hh to one accumulator that holds both products)."""
    sig, tanh = GATE_MATH[gate_math]
    L, B, H = h0.shape
    lens = [int(T)] * B if isinstance(T, int) else [int(n) for n in T]
    assert len(lens) == B and _num_layers(params) == L
    x = h0.new_zeros(B, H)
    h, c = list(h0.unbind(0)), list(c0.unbind(0))
    outs = []
    for t in range(max(lens)):
        for l in range(L):
            if matmul is None:
                gx = F.linear(x, params[f"weight_ih_l{l}"], params[f"bias_ih_l{l}"])
            else:
                gx = (params[f"bias_ih_l{l}"] + params[f"bias_hh_l{l}"]) + matmul(x, params[f"weight_ih_l{l}"], "ih")
            h[l], c[l] = _lstm_cell(gx, h[l], c[l], params[f"weight_hh_l{l}"], params[f"bias_hh_l{l}"], sig, tanh, matmul)
            x = h[l]
        outs.append(x)
    seq = torch.stack(outs)                                                          # (T_max, B, H)
    if recons is None:
        return [seq[:n, b] for b, n in enumerate(lens)]
    return [torch.flip(F.linear(seq[:n, b], recons[0], recons[1]), (0,)) for b, n in enumerate(lens)]


def bigru_scores(x, p, prefix, head_w, head_b, gru):
    h, _ = gru(x)
    return torch.sigmoid(F.linear(h, p[head_w], p[head_b]))
