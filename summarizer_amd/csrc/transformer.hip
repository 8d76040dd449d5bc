// Transformer-encoder scorer (inference) for a packed batch of videos on gfx950.
// Reference: summarizer/models/transformer.py:74-103 -- stock nn.TransformerEncoder (post-norm layers: multi-head
// self-attention, residual, LayerNorm, ReLU feed-forward, residual, LayerNorm), final norm = the SHARED layer_norm,
// optional extra residual, then k1 + ReLU + the same layer_norm + k2 + sigmoid.
//
// Built from the kernels of the VASNet path: every projection is the fp32 MFMA GEMM (bias / bias+ReLU / bias+residual fused
// in its epilogue); per-(video, head) logits and context are grouped GEMMs over a device table with one sub-problem per
// (video, head) that address Q/K/V head slices in place (ld = 3D) and write the context straight into the concatenated
// (frames, D) layout; softmax is one wave per (query row, head) with shuffle reductions.
// Inference in bf16x6 / bf16x3 with the weights' planes given (round 5): every projection on the plane GEMM (gemm_pw.hip), and -- heads of 128
// columns, videos of at most 320 frames -- the per-head attention on the multi-head form of attn_pw.hip; see "plane path" below.
#include "tf_internal.h"
#include <math.h>
#include <algorithm>

namespace sumk {

// Plane path (inference in bf16x6 / bf16x3; gemm_pw.hip): every projection of the stack reads bf16 planes of both operands.  The
// weights' planes are built once per weight change (sumk_transformer_wplanes_build: per layer [Win | Wo | W1 | W2], then k1), the
// activations' by split_planes (layer input, context, LayerNorm output) or by the producing epilogue (ReLU(lin1): PW_PLANES with bias +
// ReLU, never stored as fp32).  Two plane buffers behind the regular carve-up (sumk_transformer_workspace_bytes_for).
struct TfWPlanes { size_t win, wo, w1, w2, lay_stride, k1, total; };
static bool tf_wplanes_ok(int D, int F, int np) {
  return (np == 2 || np == 3) && D >= 256 && D % 256 == 0 && F >= 256 && F % 256 == 0 && pw_ok(256, 3 * (int64_t)D, D, 256, 3 * (int64_t)D, np) &&
         pw_ok(256, F, D, 256, F, np) && pw_ok(256, D, F, 256, D, np);
}
static TfWPlanes tf_wplanes_layout(int D, int F, int n_layers, int np) {
  TfWPlanes l; size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  l.win = take(pw_planes_bytes(3 * (int64_t)D, D, np)); l.wo = take(pw_planes_bytes(D, D, np));
  l.w1 = take(pw_planes_bytes(F, D, np)); l.w2 = take(pw_planes_bytes(D, F, np));
  l.lay_stride = p; l.k1 = p * (size_t)n_layers;
  l.total = l.k1 + align_up(pw_planes_bytes(D, D, np), 256);
  return l;
}
// ... and, when the batch is eligible, the attention on planes too (TfPwExtra, tf_internal.h)
static TfPwExtra tf_pw_extra(int D, int F, int64_t R, int np, size_t base, int heads, int n_seq, int t_max) {
  TfPwExtra e; size_t p = align_up(base, 256); e.t_max = t_max;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  e.pa = take(pw_planes_bytes(R, std::max(D, F), np)); e.pb = take(pw_planes_bytes(R, std::max(D, F), np));
  e.attn = attn_pw_heads_ok(t_max, D, heads, R, np);
  e.qp = e.ap = e.seqinfo = 0;
  if (e.attn) {
    e.qp = take(pw_planes_bytes(R, 3 * D, np)); e.ap = take((size_t)heads * align_up(pw_alpha_bytes(R, t_max, np), 256));
    e.seqinfo = take((size_t)n_seq * sizeof(SeqInfo));
  }
  e.total = p;
  return e;
}
static int tf_t_max(int n_seq, const int32_t* off) {
  int t = 0;
  for (int s = 0; s < n_seq; ++s) t = std::max(t, off[s + 1] - off[s]);
  return t;
}
__global__ void tf_seqinfo_kernel(const int32_t* off, int n_seq, SeqInfo* out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  SeqInfo si; si.eoff = 0; si.row0 = off[s]; si.T = off[s + 1] - off[s]; si.ldE = (si.T + 3) & ~3; si.pad_ = 0; si.e16off = 0;
  out[s] = si;
}
static int tf_np(int precision) { return precision == SUMK_PRECISION_BF16X6 ? 3 : precision == SUMK_PRECISION_BF16X3 ? 2 : 0; }
static bool tf_pw_rows_ok(int D, int F, int64_t R, int np) {
  return R >= 128 && pw_ok(R, 3 * (int64_t)D, D, R, 3 * (int64_t)D, np) && pw_ok(R, F, D, R, F, np) && pw_ok(R, D, F, R, D, np);
}
// logits = false: the carves of the stream path -- no `e`, `seq` or `prob_tabs`, in training no `l_p` / `l_pd` either; attn_stream.hip's
// descriptors instead, in training with attn_stream_bwd.hip's delta behind them and the attention statistic among the per-layer saves
static int tf_carve_any(int D, int F, int heads, int n_layers, int n_seq, const int32_t* off, int training, bool logits, TfWs* w) {
  SUMK_ARG(D > 0 && D % 4 == 0 && F > 0 && F % 4 == 0, "transformer: D=%d / F=%d must be positive multiples of 4", D, F);
  SUMK_ARG(heads > 0 && D % heads == 0 && (D / heads) % 4 == 0, "transformer: head dim must be a multiple of 4 (D=%d heads=%d)", D, heads);
  SUMK_ARG(n_seq > 0 && off && off[0] == 0, "transformer: empty batch / seq_off[0] != 0");
  int64_t e = 0;
  for (int s = 0; s < n_seq; ++s) {
    int T = off[s + 1] - off[s];
    SUMK_ARG(T > 0, "transformer: video %d has %d frames", s, T);
    SUMK_ARG(T < (1 << 20), "transformer: video %d has %d frames (limit 2^20)", s, T);
    e += (int64_t)heads * T * ((T + 3) & ~3);
  }
  const size_t R = (size_t)off[n_seq];
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  w->n_rows = (int32_t)R; w->e_elems = e;
  w->seq = w->prob_tabs = w->e = w->l_p = w->l_pd = w->l_astats = w->as_seq = 0;
  if (logits) w->seq = take((size_t)n_seq * sizeof(TfSeq));
  w->prob_row = take(8 * sizeof(GemmProb));
  if (logits) w->prob_tabs = take((size_t)TT_COUNT * n_seq * heads * sizeof(GemmProb));   // (the stream path has no per-(video, head) GEMMs)
  w->t1 = take(R * D * 4);
  if (!training) {
    w->qkv = take(R * 3 * D * 4);
    if (logits) w->e = take((size_t)e * 4); else w->as_seq = take(attn_stream_ws_bytes(n_seq));
    w->ctx = take(R * D * 4);
    w->h0 = take(R * D * 4); w->h1 = take(R * D * 4); w->h2 = take(R * D * 4); w->ff = take(R * (size_t)F * 4);
  } else {
    size_t q = 0;
    auto lt = [&](size_t bytes) { size_t at = q; q += align_up(bytes, 256); return at; };
    w->l_qkv = lt(R * 3 * D * 4);
    if (logits) { w->l_p = lt((size_t)e * 4); w->l_pd = lt((size_t)e * 4); } else w->l_astats = lt(R * (size_t)heads * 8);
    w->l_ctx = lt(R * D * 4);
    w->l_t1a = lt(R * D * 4); w->l_hmid = lt(R * D * 4); w->l_ff = lt(R * (size_t)F * 4); w->l_t1b = lt(R * D * 4);
    w->l_hout = lt(R * D * 4); w->l_stats = lt(R * 4 * 4);
    w->lay_stride = q;
    w->lay0 = take(q * (size_t)n_layers);
    if (!logits) w->as_seq = take(attn_stream_bwd_ws_bytes(heads, n_seq, (int64_t)R));
    w->hfin = take(R * D * 4); w->z = take(R * D * 4); w->stats_fin = take(R * 4 * 4); w->scores = take(R * 4);
    w->g0 = take(R * D * 4); w->g1 = take(R * D * 4); w->g2 = take(R * D * 4);
    w->dqkv = take(R * 3 * D * 4); w->dff = take(R * (size_t)F * 4);
    w->lnpart = take((size_t)(LNB_MAX_WAVES / 4) * ln_slot_floats(D) * 4);
    w->colpart = take((size_t)TF_COLSUM_CHUNKS * 3 * D * 4 + (size_t)TF_COLSUM_CHUNKS * F * 4);
    w->slab_elems = (size_t)24 * D * std::max(D, F);
    w->slab = take(w->slab_elems * 4);
    w->prob_sk = take(TF_SPLITK_PROBS * sizeof(GemmProb));
  }
  w->total = p;
  return SUMK_OK;
}
int tf_carve(int D, int F, int heads, int n_layers, int n_seq, const int32_t* off, int training, TfWs* w) {
  return tf_carve_any(D, F, heads, n_layers, n_seq, off, training, true, w);
}

__global__ void tf_setup_kernel(const int32_t* off, int n_seq, int D, int heads, TfSeq* seq, GemmProb* tabs) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  const int dh = D / heads, bt = 64, tnv = (dh + bt - 1) / bt, np = n_seq * heads;
  int64_t eoff = 0; int ts = 0, tpv = 0;
  for (int q = 0; q < s; ++q) {
    int T = off[q + 1] - off[q], tm = (T + bt - 1) / bt;
    eoff += (int64_t)heads * T * ((T + 3) & ~3); ts += heads * tm * tm; tpv += heads * tm * tnv;
  }
  const int row0 = off[s], T = off[s + 1] - row0, ldE = (T + 3) & ~3, tm = (T + bt - 1) / bt;
  TfSeq si; si.eoff = eoff; si.row0 = row0; si.T = T; si.ldE = ldE; si.pad_ = 0;
  seq[s] = si;
  auto put = [&](int tab, int h, int64_t a_off, int64_t b_off, int64_t c_off, int M, int N, int K, int lda, int ldb, int ldc,
                 int tile_start, int tiles_n) {
    GemmProb q;
    q.a_off = a_off; q.b_off = b_off; q.c_off = c_off; q.r_off = 0;
    q.M = M; q.N = N; q.K = K; q.lda = lda; q.ldb = ldb; q.ldc = ldc; q.ldr = 0; q.tile_start = tile_start; q.tiles_n = tiles_n;
    for (int i = 0; i < 7; ++i) q.pad_[i] = 0;
    tabs[(size_t)tab * np + s * heads + h] = q;
  };
  for (int h = 0; h < heads; ++h) {
    const int64_t q0 = (int64_t)row0 * 3 * D + h * dh, eb = eoff + (int64_t)h * T * ldE, c0 = (int64_t)row0 * D + h * dh;
    const int t_s = ts + h * tm * tm, t_pv = tpv + h * tm * tnv;
    put(TT_S, h, q0, q0 + D, eb, T, T, dh, 3 * D, 3 * D, ldE, t_s, tm);              // E = Q_h K_h^T          (NT, K = dh)
    put(TT_PV, h, eb, q0 + 2 * D, c0, T, dh, T, ldE, 3 * D, D, t_pv, tnv);           // C_h = alpha_h V_h      (NN, K = T)
    put(TT_DV, h, eb, c0, q0 + 2 * D, T, dh, T, ldE, D, 3 * D, t_pv, tnv);           // dV_h = alpha_h^T dC_h  (TN)
    put(TT_DP, h, c0, q0 + 2 * D, eb, T, T, dh, D, 3 * D, ldE, t_s, tm);             // dAlpha = dC_h V_h^T    (NT)
    put(TT_DQ, h, eb, q0 + D, q0, T, dh, T, ldE, 3 * D, 3 * D, t_pv, tnv);           // dQ_h = dS K_h          (NN)
    put(TT_DK, h, eb, q0, q0 + D, T, dh, T, ldE, 3 * D, 3 * D, t_pv, tnv);           // dK_h = dS^T Q_h        (TN)
  }
}

// one wave per (query row, head): alpha = softmax(scale * logits); pad columns zeroed; training with dropout also writes
// dropout(alpha) to E2 (mask index = ((row*heads + h) << 20) | j)
__global__ __launch_bounds__(256) void tf_softmax_kernel(float* E, float* E2, const TfSeq* seq, const int32_t* off, int n_seq,
                                                         int n_rows, int heads, float scale, Drop drop, uint32_t site) {
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (int64_t)n_rows * heads) return;
  const int lane = threadIdx.x & 63;
  const int row = (int)(wid / heads), h = (int)(wid % heads);
  int lo = 0, hi = n_seq - 1;
  while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (off[mid] <= row) lo = mid; else hi = mid - 1; }
  const TfSeq si = seq[lo];
  const int i = row - si.row0, T = si.T;
  const int64_t ro = si.eoff + ((int64_t)h * T + i) * si.ldE;
  float* e = E + ro;
  if (T <= 512) {        // the row lives in registers: one read, one exp per element (same operations in the same order as the loops below)
    float v[8];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int j = lane + 64 * q; v[q] = j < T ? e[j] : -INFINITY; }
#pragma unroll
    for (int q = 0; q < 8; ++q) m = fmaxf(m, v[q] * scale);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (lane + 64 * q < T) { v[q] = expf(__builtin_fmaf(v[q], scale, -m)); sum += v[q]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = lane + 64 * q;
      if (j < si.ldE) {
        const float a = j < T ? v[q] / sum : 0.f;
        e[j] = a;
        if (E2) E2[ro + j] = drop.thr ? drop_apply(drop, site, ((uint64_t)wid << 20) | (uint64_t)j, a) : a;
      }
    }
    return;
  }
  float m = -INFINITY;
  for (int j = lane; j < T; j += 64) m = fmaxf(m, e[j] * scale);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float sum = 0.f;
  for (int j = lane; j < T; j += 64) sum += expf(__builtin_fmaf(e[j], scale, -m));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  for (int j = lane; j < si.ldE; j += 64) {
    const float v = j < T ? expf(__builtin_fmaf(e[j], scale, -m)) / sum : 0.f;
    e[j] = v;
    if (E2) E2[ro + j] = drop.thr ? drop_apply(drop, site, ((uint64_t)wid << 20) | (uint64_t)j, v) : v;
  }
}

// dLogits = scale * alpha * (dAlpha - sum_j dAlpha_j alpha_j), dAlpha = dropout'(dAlphaDropped); in place on E2
__global__ __launch_bounds__(256) void tf_softmax_bwd_kernel(const float* E, float* E2, const TfSeq* seq, const int32_t* off,
                                                             int n_seq, int n_rows, int heads, float scale, Drop drop,
                                                             uint32_t site) {
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (int64_t)n_rows * heads) return;
  const int lane = threadIdx.x & 63;
  const int row = (int)(wid / heads), h = (int)(wid % heads);
  int lo = 0, hi = n_seq - 1;
  while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (off[mid] <= row) lo = mid; else hi = mid - 1; }
  const TfSeq si = seq[lo];
  const int i = row - si.row0, T = si.T;
  const int64_t ro = si.eoff + ((int64_t)h * T + i) * si.ldE;
  const float* p = E + ro; float* g = E2 + ro;
  float dot = 0.f;
  for (int j = lane; j < T; j += 64) {
    float d = g[j];
    if (drop.thr) d = drop_apply(drop, site, ((uint64_t)wid << 20) | (uint64_t)j, d);
    dot += d * p[j];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
  for (int j = lane; j < si.ldE; j += 64) {
    float v = 0.f;
    if (j < T) {
      float d = g[j];
      if (drop.thr) d = drop_apply(drop, site, ((uint64_t)wid << 20) | (uint64_t)j, d);
      v = p[j] * (d - dot) * scale;
    }
    g[j] = v;
  }
}

__global__ void add_rows_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t n4) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  float4 a = reinterpret_cast<float4*>(y)[i], b = reinterpret_cast<const float4*>(x)[i];
  a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  reinterpret_cast<float4*>(y)[i] = a;
}
// dst[r,c] = src[r,c] * (keep(site, r*N + c) ? scale : 0)      (backward of an epilogue dropout)
__global__ void mask_scale_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n, Drop drop, uint32_t site) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = drop_apply(drop, site, (uint64_t)i, src[i]);
}
// g[i] = act[i] > 0 ? g[i] * scale : 0   -- backward of dropout(relu(.)) given the stored post-dropout activation
__global__ void relu_drop_bwd_kernel(float* __restrict__ g, const float* __restrict__ act, int64_t n, float scale) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g[i] = act[i] > 0.f ? g[i] * scale : 0.f;
}

static int tf_geometry_any(int D, int F, int heads, int n_layers, int n_seq, const int32_t* off, int training, bool logits, TfGeom* G) {
  SUMK_TRY(tf_carve_any(D, F, heads, n_layers, n_seq, off, training, logits, &G->L));
  G->R = G->L.n_rows; G->dh = D / heads; G->tiles_s = G->tiles_pv = 0;
  for (int s = 0; logits && s < n_seq; ++s) {
    int T = off[s + 1] - off[s], tm = (T + 63) / 64;
    G->tiles_s += heads * tm * tm; G->tiles_pv += heads * tm * ((G->dh + 63) / 64);
  }
  auto cfg = [&](int M, int N) { return gemm_tiles(M, N, 0) >= 512 ? 0 : 1; };
  G->c_qkv = cfg(G->R, 3 * D); G->c_dd = cfg(G->R, D); G->c_df = cfg(G->R, F);
  return SUMK_OK;
}
int tf_geometry(int D, int F, int heads, int n_layers, int n_seq, const int32_t* off, int training, TfGeom* G) {
  return tf_geometry_any(D, F, heads, n_layers, n_seq, off, training, true, G);
}

int tf_plan(const char* what, int attn, int training, int attn_prec, int D, int F, int heads, int n_layers, int n_seq, const int32_t* off_host,
            const sumk_tf_opts* opts, TfPlan* P) {
  P->stream = attn != TF_DENSE; P->training = training != 0; P->attn_prec = attn == TF_STREAM_SPLIT ? attn_prec : 0; P->planes = 0; P->px = TfPwExtra{};
  SUMK_ARG(n_layers >= 1, "%s: n_layers=%d", what, n_layers);
  SUMK_ARG(attn != TF_STREAM_SPLIT || attn_prec == SUMK_PRECISION_BF16X3, "%s: attention_precision=%d (only SUMK_PRECISION_BF16X3 = %d)", what,
           attn_prec, SUMK_PRECISION_BF16X3);
  SUMK_TRY(tf_geometry_any(D, F, heads, n_layers, n_seq, off_host, P->training, !P->stream, &P->G));
  P->tail = P->G.L.total; P->tail_bytes = 0;
  if (P->stream) {
    SUMK_ARG(!opts || (opts->precision == SUMK_PRECISION_FP32 && !opts->wplanes), "%s: exact fp32 only (precision=%d, wplanes %s)", what,
             opts->precision, opts->wplanes ? "given" : "null");
    SUMK_TRY(P->training ? attn_stream_bwd_check(D, heads, n_seq, off_host) : attn_stream_check(D, heads, n_seq, off_host));
    if (P->attn_prec) {   // one layer's descriptors, (training: delta) and planes; a refusal's message is the attention unit's
      P->tail_bytes = P->training ? attn_stream_split_bwd_ws_bytes(D, heads, n_seq, off_host, P->attn_prec)
                                  : attn_stream_split_ws_bytes(D, heads, n_seq, off_host, P->attn_prec);
      if (!P->tail_bytes) return SUMK_ERR_ARG;
    }
  }
  if (opts && (opts->layer_dropout_p != 0.f || opts->head_dropout_p != 0.f))
    SUMK_ARG(P->training, P->stream ? "%s: inference only (dropout must be 0)" : "%s: dropout needs training mode", what);
  const int np = opts && opts->wplanes ? tf_np(opts->precision) : 0;
  if (!P->stream && !P->training && np && tf_wplanes_ok(D, F, np) && tf_pw_rows_ok(D, F, P->G.R, np)) {
    P->planes = np;
    P->px = tf_pw_extra(D, F, P->G.R, np, P->tail, heads, n_seq, tf_t_max(n_seq, off_host));
    P->tail_bytes = P->px.total - P->tail;
  }
  P->total = P->tail + P->tail_bytes;
  return SUMK_OK;
}

int tf_tables(const TfGeom& G, int D, int F, int heads, int n_seq, const int32_t* off_dev, char* ws, hipStream_t stream, bool head_tables) {
  const int R = G.R;
  GemmProb* prow = (GemmProb*)(ws + G.L.prob_row);
  if (head_tables)
    hipLaunchKernelGGL(tf_setup_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, off_dev, n_seq, D, heads,
                       (TfSeq*)(ws + G.L.seq), (GemmProb*)(ws + G.L.prob_tabs));
  SUMK_TRY(fill_single_prob(prow + P_QKV, R, 3 * D, D, D, D, 3 * D, 0, G.c_qkv, stream));   // (R,3D) <- (R,D) x (3D,D)^T
  SUMK_TRY(fill_single_prob(prow + P_DD, R, D, D, D, D, D, D, G.c_dd, stream));             // (R,D)  <- (R,D) x (D,D)   [+R ld D]
  SUMK_TRY(fill_single_prob(prow + P_DF, R, F, D, D, D, F, 0, G.c_df, stream));             // (R,F)  <- (R,D) x (F,D)^T ; also NN with B (D,F)
  SUMK_TRY(fill_single_prob(prow + P_FD, R, D, F, F, F, D, D, G.c_dd, stream));             // (R,D)  <- (R,F) x (D,F)^T ; NN with B (F,D): ldb = D set below
  SUMK_TRY(fill_single_prob(prow + P_DQKV, R, D, 3 * D, 3 * D, D, D, D, G.c_dd, stream));   // (R,D)  <- (R,3D) x (3D,D)  (NN)
  SUMK_TRY(fill_single_prob(prow + P_NN_DF, R, F, D, D, F, F, 0, G.c_df, stream));          // (R,F)  <- (R,D) x (D,F)    (NN)
  SUMK_TRY(fill_single_prob(prow + P_NN_FD, R, D, F, F, D, D, D, G.c_dd, stream));          // (R,D)  <- (R,F) x (F,D)    (NN)
  return SUMK_OK;
}


// ---- exact-fp32 blocks of one post-norm layer (tf_internal.h), shared with the encoder / decoder stack entries (tf_decoder.hip)
int tf_in_proj(const TfRun& r, const float* hin, const float* in_w, const float* in_b, float* QKV) {
  const TfGeom& G = *r.G; const int R = G.R, D = r.D;
  GemmLaunch g; g.precision = r.precision;
  g.A = hin; g.B[0] = in_w; g.bias0[0] = in_b; g.C = QKV; g.probs = (const GemmProb*)(r.ws + G.L.prob_row) + P_QKV; g.small_tile = G.c_qkv;
  g.total_tiles = gemm_tiles(R, 3 * D, G.c_qkv); g.xcd_M = R; g.xcd_N = 3 * D; g.lean = gemm_lean_ok(R, 3 * D, D, D, D);
  return launch_gemm(GEMM_NT, EPI_BIAS2, g, r.stream);
}

int tf_out_proj(const TfRun& r, const float* CTX, const float* out_w, const float* out_b, const float* hres, float* T, Drop dl,
                uint32_t site) {
  const TfGeom& G = *r.G; const int R = G.R, D = r.D;
  GemmLaunch g; g.precision = r.precision;
  g.A = CTX; g.B[0] = out_w; g.bias0[0] = out_b; g.R = hres; g.C = T; g.probs = (const GemmProb*)(r.ws + G.L.prob_row) + P_DD;
  g.small_tile = G.c_dd; g.total_tiles = gemm_tiles(R, D, G.c_dd); g.xcd_M = R; g.xcd_N = D; g.lean = gemm_lean_ok(R, D, D, D, D);
  g.drop_seed = dl.seed; g.drop_thr = dl.thr; g.drop_scale = dl.scale; g.drop_site = site;
  return launch_gemm(GEMM_NT, EPI_BIAS_RESIDUAL, g, r.stream);
}

int tf_attn_core_fwd(const TfRun& r, const GemmProb* tabs, const float* qbase, const float* kvbase, float* E, float* E2, float* CTX,
                     Drop dl, uint32_t site) {
  const TfGeom& G = *r.G; const int R = G.R, np = r.n_seq * r.heads;
  prof_begin(SUMK_PROF_TF_ATTN_DENSE, r.stream);
  {  // logits per (video, head)
    GemmLaunch g; g.precision = r.precision;
    g.A = qbase; g.B[0] = kvbase; g.C = E; g.probs = tabs + (size_t)TT_S * np; g.nprob = np; g.small_tile = 1; g.total_tiles = G.tiles_s;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_NONE, g, r.stream));
  }
  hipLaunchKernelGGL(tf_softmax_kernel, dim3((unsigned)(((int64_t)R * r.heads + 3) / 4)), dim3(256), 0, r.stream, E,
                     dl.thr ? E2 : nullptr, (const TfSeq*)(r.ws + G.L.seq), r.off_dev, r.n_seq, R, r.heads,
                     1.0f / sqrtf((float)G.dh), dl, site);
  {  // context, heads written side by side
    GemmLaunch g; g.precision = r.precision;
    g.A = dl.thr ? E2 : E; g.B[0] = kvbase; g.C = CTX; g.probs = tabs + (size_t)TT_PV * np; g.nprob = np; g.small_tile = 1;
    g.total_tiles = G.tiles_pv;
    SUMK_TRY(launch_gemm(GEMM_NN, EPI_NONE, g, r.stream));
  }
  prof_end(SUMK_PROF_TF_ATTN_DENSE, r.stream);
  return SUMK_OK;
}

int tf_attn_core_bwd(const TfRun& r, const GemmProb* tabs, const float* qbase, const float* kvbase, const float* P, float* E2,
                     const float* dCTX, float* dq_base, float* dkv_base, Drop dl, uint32_t site) {
  const TfGeom& G = *r.G; const int R = G.R, np = r.n_seq * r.heads;
  const float* Pd = dl.thr ? (const float*)E2 : P;
  {
    GemmLaunch g; g.precision = r.precision;
    g.A = Pd; g.B[0] = dCTX; g.C = dkv_base; g.probs = tabs + (size_t)TT_DV * np; g.nprob = np; g.small_tile = 1; g.total_tiles = G.tiles_pv;
    SUMK_TRY(launch_gemm(GEMM_TN, EPI_NONE, g, r.stream));
  }
  {
    GemmLaunch g; g.precision = r.precision;
    g.A = dCTX; g.B[0] = kvbase; g.C = E2; g.probs = tabs + (size_t)TT_DP * np; g.nprob = np; g.small_tile = 1; g.total_tiles = G.tiles_s;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_NONE, g, r.stream));
  }
  hipLaunchKernelGGL(tf_softmax_bwd_kernel, dim3((unsigned)(((int64_t)R * r.heads + 3) / 4)), dim3(256), 0, r.stream, P, E2,
                     (const TfSeq*)(r.ws + G.L.seq), r.off_dev, r.n_seq, R, r.heads, 1.0f / sqrtf((float)G.dh), dl, site);
  {
    GemmLaunch g; g.precision = r.precision;
    g.A = E2; g.B[0] = kvbase; g.C = dq_base; g.probs = tabs + (size_t)TT_DQ * np; g.nprob = np; g.small_tile = 1; g.total_tiles = G.tiles_pv;
    SUMK_TRY(launch_gemm(GEMM_NN, EPI_NONE, g, r.stream));
  }
  {
    GemmLaunch g; g.precision = r.precision;
    g.A = E2; g.B[0] = qbase; g.C = dkv_base; g.probs = tabs + (size_t)TT_DK * np; g.nprob = np; g.small_tile = 1; g.total_tiles = G.tiles_pv;
    SUMK_TRY(launch_gemm(GEMM_TN, EPI_NONE, g, r.stream));
  }
  return SUMK_OK;
}

int tf_attn_stream_fwd(const TfRun& r, const float* QKV, float* CTX, float* astats, Drop dl, uint32_t site) {
  const int D = r.D, prec = r.plan->attn_prec; const float scale = 1.0f / sqrtf((float)r.G->dh);
  char* const split_ws = r.ws + r.plan->tail; char* const as_seq = r.ws + r.G->L.as_seq;
  if (!astats)   // scoring: no statistic, no masks
    return prec ? launch_attn_stream_split(QKV, 3 * D, QKV + D, 3 * D, QKV + 2 * D, 3 * D, D, r.heads, r.n_seq, r.off_host, r.off_dev, scale, prec,
                                           CTX, D, nullptr, split_ws, r.stream)
                : launch_attn_stream(QKV, 3 * D, QKV + D, 3 * D, QKV + 2 * D, 3 * D, D, r.heads, r.n_seq, r.off_host, r.off_dev, scale, CTX, D,
                                     nullptr, as_seq, r.stream);
  return prec ? launch_attn_stream_split_train(QKV, 3 * D, QKV + D, 3 * D, QKV + 2 * D, 3 * D, D, r.heads, r.n_seq, r.off_host, r.off_dev, scale,
                                               prec, dl, site, CTX, D, astats, split_ws, r.stream)
              : launch_attn_stream_train(QKV, 3 * D, QKV + D, 3 * D, QKV + 2 * D, 3 * D, D, r.heads, r.n_seq, r.off_host, r.off_dev, scale, dl, site,
                                         CTX, D, astats, as_seq, r.stream);
}

int tf_attn_stream_bwd(const TfRun& r, const float* QKV, const float* CTX, const float* dCTX, const float* astats, float* dQKV, Drop dl,
                       uint32_t site) {
  const int D = r.D;
  if (r.plan->attn_prec)
    return launch_attn_stream_split_bwd(QKV, 3 * D, QKV + D, 3 * D, QKV + 2 * D, 3 * D, CTX, D, dCTX, D, astats, D, r.heads, r.n_seq, r.off_host,
                                        r.off_dev, 1.0f / sqrtf((float)r.G->dh), r.plan->attn_prec, dl, site, dQKV, 3 * D, dQKV + D, 3 * D,
                                        dQKV + 2 * D, 3 * D, r.ws + r.plan->tail, r.stream);
  return launch_attn_stream_bwd(QKV, 3 * D, QKV + D, 3 * D, QKV + 2 * D, 3 * D, CTX, D, dCTX, D, astats, D, r.heads, r.n_seq, r.off_host,
                                r.off_dev, 1.0f / sqrtf((float)r.G->dh), dl, site, dQKV, 3 * D, dQKV + D, 3 * D, dQKV + 2 * D, 3 * D,
                                r.ws + r.G->L.as_seq, r.stream);
}

int tf_sa_fwd(const TfRun& r, const TfAttnW& W, const float* hin, float* QKV, float* E, float* E2, float* CTX, float* T1a, Drop dl,
              uint32_t site, float* astats) {
  SUMK_TRY(tf_in_proj(r, hin, W.in_w, W.in_b, QKV));
  if (r.plan && r.plan->stream) SUMK_TRY(tf_attn_stream_fwd(r, QKV, CTX, astats, dl, site + 0));
  else SUMK_TRY(tf_attn_core_fwd(r, (const GemmProb*)(r.ws + r.G->L.prob_tabs), QKV, QKV, E, E2, CTX, dl, site + 0));
  return tf_out_proj(r, CTX, W.out_w, W.out_b, hin, T1a, dl, site + 1);
}

int tf_wgrad(const TfRun& r, const float* dY, int ldy, int M, const float* Xin, int ldx, int N, float* out) {
  const TfWs& L = r.G->L;
  float* outs[4] = {out, nullptr, nullptr, nullptr};
  return gemm_tn_splitk_accum(dY, ldy, Xin, ldx, M, N, r.G->R, (float*)(r.ws + L.slab), L.slab_elems, (GemmProb*)(r.ws + L.prob_sk),
                              TF_SPLITK_PROBS, outs, M, N, 1.f, r.stream, r.precision);
}

int tf_nn(const TfRun& r, const float* A, const float* B, float* C, int prob, GemmEpi epi, int N) {
  const TfGeom& G = *r.G;
  GemmLaunch g; g.precision = r.precision;
  g.A = A; g.B[0] = B; g.C = C; g.probs = (const GemmProb*)(r.ws + G.L.prob_row) + prob; g.small_tile = (N == r.F ? G.c_df : G.c_dd);
  g.total_tiles = gemm_tiles(G.R, N, g.small_tile);
  return launch_gemm(GEMM_NN, epi, g, r.stream);
}

static dim3 tf_blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

int tf_sa_bwd(const TfRun& r, const TfAttnW& W, const TfAttnG& Gd, const float* hin, const float* QKV, const float* P, float* E2,
              const float* CTX, float* dT, float* s1, float* s2, float* dQKV, Drop dl, uint32_t site, const float* astats) {
  const int R = r.G->R, D = r.D; const int64_t nRD = (int64_t)R * D;
  float* colpart = (float*)(r.ws + r.G->L.colpart);
  const float* dAO = dT;
  if (dl.thr) { hipLaunchKernelGGL(mask_scale_kernel, tf_blocks(nRD), dim3(256), 0, r.stream, s2, dT, nRD, dl, site + 1); dAO = s2; }
  SUMK_TRY(colsum_accum(dAO, D, R, D, colpart, TF_COLSUM_CHUNKS, Gd.out_b, r.stream));
  SUMK_TRY(tf_wgrad(r, dAO, D, D, CTX, D, D, Gd.out_w));
  SUMK_TRY(tf_nn(r, dAO, W.out_w, s1, P_DD, EPI_NONE, D));                  // s1 = dCTX
  // multi-head attention backward, per (video, head)
  if (astats) SUMK_TRY(tf_attn_stream_bwd(r, QKV, CTX, s1, astats, dQKV, dl, site + 0));
  else SUMK_TRY(tf_attn_core_bwd(r, (const GemmProb*)(r.ws + r.G->L.prob_tabs), QKV, QKV, P, E2, s1, dQKV, dQKV, dl, site + 0));
  SUMK_TRY(colsum_accum(dQKV, 3 * D, R, 3 * D, colpart, TF_COLSUM_CHUNKS, Gd.in_b, r.stream));
  SUMK_TRY(tf_wgrad(r, dQKV, 3 * D, 3 * D, hin, D, D, Gd.in_w));
  return tf_nn(r, dQKV, W.in_w, dT, P_DQKV, EPI_ACCUM, D);                  // dHin = dT1a + dQKV . Win   (Win stored (3D,D) = (K,N))
}

int tf_ff_fwd(const TfRun& r, const TfFfW& W, const float* h, float* FF, float* T, Drop dl, uint32_t site_a, uint32_t site_b) {
  const TfGeom& G = *r.G; const int R = G.R, D = r.D, F = r.F;
  const GemmProb* prow = (const GemmProb*)(r.ws + G.L.prob_row);
  {  // feed-forward 1: bias + ReLU (+dropout)
    GemmLaunch g; g.precision = r.precision;
    g.A = h; g.B[0] = W.w1; g.bias0[0] = W.b1; g.C = FF; g.probs = prow + P_DF; g.small_tile = G.c_df;
    g.total_tiles = gemm_tiles(R, F, G.c_df); g.xcd_M = R; g.xcd_N = F; g.lean = gemm_lean_ok(R, F, D, D, D);
    g.drop_seed = dl.seed; g.drop_thr = dl.thr; g.drop_scale = dl.scale; g.drop_site = site_a;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_BIAS_RELU, g, r.stream));
  }
  {  // feed-forward 2: bias (+dropout) + residual
    GemmLaunch g; g.precision = r.precision;
    g.A = FF; g.B[0] = W.w2; g.bias0[0] = W.b2; g.R = h; g.C = T; g.probs = prow + P_FD; g.small_tile = G.c_dd;
    g.total_tiles = gemm_tiles(R, D, G.c_dd); g.xcd_M = R; g.xcd_N = D; g.lean = gemm_lean_ok(R, D, F, F, F);
    g.drop_seed = dl.seed; g.drop_thr = dl.thr; g.drop_scale = dl.scale; g.drop_site = site_b;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_BIAS_RESIDUAL, g, r.stream));
  }
  return SUMK_OK;
}

int tf_ff_bwd(const TfRun& r, const TfFfW& W, const TfFfG& Gd, const float* h, const float* FFa, float* dT, float* s1, float* dFF,
              Drop dl, uint32_t site_a, uint32_t site_b) {
  (void)site_a;   // the ReLU / dropout mask of lin1 is read back from the stored post-dropout activation
  const int R = r.G->R, D = r.D, F = r.F; const int64_t nRD = (int64_t)R * D, nRF = (int64_t)R * F;
  float* colpart = (float*)(r.ws + r.G->L.colpart);
  // dT is also the residual gradient into h.  dropout mask -> s1 = d(linear2 output)
  const float* dL2 = dT;
  if (dl.thr) { hipLaunchKernelGGL(mask_scale_kernel, tf_blocks(nRD), dim3(256), 0, r.stream, s1, dT, nRD, dl, site_b); dL2 = s1; }
  SUMK_TRY(colsum_accum(dL2, D, R, D, colpart, TF_COLSUM_CHUNKS, Gd.b2, r.stream));
  SUMK_TRY(tf_wgrad(r, dL2, D, D, FFa, F, F, Gd.w2));
  SUMK_TRY(tf_nn(r, dL2, W.w2, dFF, P_NN_DF, EPI_NONE, F));                 // dFF = dL2 . W2   (W2 stored (D,F) = (K,N))
  hipLaunchKernelGGL(relu_drop_bwd_kernel, tf_blocks(nRF), dim3(256), 0, r.stream, dFF, FFa, nRF, dl.scale);
  SUMK_TRY(colsum_accum(dFF, F, R, F, colpart, TF_COLSUM_CHUNKS, Gd.b1, r.stream));
  SUMK_TRY(tf_wgrad(r, dFF, F, F, h, D, D, Gd.w1));
  return tf_nn(r, dFF, W.w1, dT, P_NN_FD, EPI_ACCUM, D);                    // dH = dT + dFF . W1   (W1 stored (F,D) = (K,N))
}

// The tail of the scorer: final (shared) LayerNorm of the encoder, optional extra residual, scoring head (k1 + ReLU on the exact-fp32
// GEMM, or -- planes = true, the dense entry's plane path -- by the caller's `k1_planes()`; then the same LayerNorm + k2 + sigmoid)
template <typename K1>
static int tf_tail(const TfRun& r, const float* x, const float* hin, float* hfin, float* Z, float* sfin, const sumk_tf_head_weights* head,
                   const sumk_tf_opts* opts, Drop dhd, float* scores, bool planes, K1 k1_planes) {
  const TfGeom& G = *r.G; const int R = G.R, D = r.D; hipStream_t stream = r.stream;
  SUMK_TRY(launch_layernorm(hin, hfin, head->ln_w, head->ln_b, R, D, opts->final_eps, sfin, stream));
  if (opts->more_residuals) {
    int64_t n4 = (int64_t)R * (D >> 2);
    hipLaunchKernelGGL(add_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, hfin, x, n4);
  }
  if (planes) {
    SUMK_TRY(k1_planes());
  } else {
    GemmLaunch g; g.precision = opts->precision;
    g.A = hfin; g.B[0] = head->k1_w; g.bias0[0] = head->k1_b; g.C = Z; g.probs = (const GemmProb*)(r.ws + G.L.prob_row) + P_DD; g.small_tile = G.c_dd;
    g.total_tiles = gemm_tiles(R, D, G.c_dd); g.xcd_M = R; g.xcd_N = D; g.lean = gemm_lean_ok(R, D, D, D, D);
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_BIAS_RELU, g, stream));
  }
  return launch_ln_head_drop(Z, head->ln_w, head->ln_b, head->k2_w, head->k2_b, scores, R, D, opts->final_eps,
                             sfin ? sfin + 2 * (size_t)R : nullptr, dhd, 1000u, stream);
}

}  // namespace sumk

using namespace sumk;

// ---- the size queries: each names its path to the plan (0 = arguments the path refuses, the reason in sumk_last_error())
static size_t tf_query(const char* what, int attn, int training, int attn_prec, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                       int32_t n_seq, const int32_t* seq_off_host, const sumk_tf_opts* opts = nullptr) {
  TfPlan P;
  return tf_plan(what, attn, training, attn_prec, D, F, n_heads, n_layers, n_seq, seq_off_host, opts, &P) == SUMK_OK ? P.total : 0;
}

extern "C" size_t sumk_transformer_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                   const int32_t* seq_off_host, int32_t training) {
  return tf_query("transformer_workspace_bytes", TF_DENSE, training, 0, D, F, n_heads, n_layers, n_seq, seq_off_host);
}

extern "C" size_t sumk_transformer_workspace_bytes_for(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                       const int32_t* seq_off_host, int32_t training, int32_t precision) {
  sumk_tf_opts o{}; o.precision = precision; o.wplanes = &o;   // a call in `precision` with the weights' planes given
  return tf_query("transformer_workspace_bytes_for", TF_DENSE, training, 0, D, F, n_heads, n_layers, n_seq, seq_off_host, &o);
}

extern "C" size_t sumk_transformer_stream_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                          const int32_t* seq_off_host) {
  return tf_query("transformer_stream_workspace_bytes", TF_STREAM, 0, 0, D, F, n_heads, n_layers, n_seq, seq_off_host);
}

extern "C" size_t sumk_transformer_stream_split_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                                const int32_t* seq_off_host, int32_t attention_precision) {
  return tf_query("transformer_stream_split_workspace_bytes", TF_STREAM_SPLIT, 0, attention_precision, D, F, n_heads, n_layers, n_seq, seq_off_host);
}

extern "C" size_t sumk_transformer_stream_train_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                                const int32_t* seq_off_host) {
  return tf_query("transformer_stream_train_workspace_bytes", TF_STREAM, 1, 0, D, F, n_heads, n_layers, n_seq, seq_off_host);
}

extern "C" size_t sumk_transformer_stream_split_train_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                                      const int32_t* seq_off_host, int32_t attention_precision) {
  return tf_query("transformer_stream_split_train_workspace_bytes", TF_STREAM_SPLIT, 1, attention_precision, D, F, n_heads, n_layers, n_seq,
                  seq_off_host);
}

extern "C" size_t sumk_transformer_wplanes_bytes(int32_t D, int32_t F, int32_t n_layers, int32_t n_planes) {
  if (n_layers < 1 || D < 1 || F < 1 || !tf_wplanes_ok(D, F, n_planes)) return 0;
  return tf_wplanes_layout(D, F, n_layers, n_planes).total;
}

extern "C" int sumk_transformer_wplanes_build(int32_t D, int32_t F, int32_t n_layers, const sumk_tf_layer_weights* layers,
                                              const sumk_tf_head_weights* head, int32_t n_planes, void* out, size_t out_bytes,
                                              void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(layers && head && out && n_layers > 0, "transformer_wplanes_build: null pointer");
  SUMK_ARG(tf_wplanes_ok(D, F, n_planes), "transformer_wplanes_build: D=%d F=%d planes=%d is not eligible (D, F multiples of 256; 2 or 3 planes)", D, F, n_planes);
  const TfWPlanes l = tf_wplanes_layout(D, F, n_layers, n_planes);
  SUMK_ARG(out_bytes >= l.total && ((uintptr_t)out & 255) == 0, "transformer_wplanes_build: %zu bytes (256-byte aligned) needed, got %zu", l.total, out_bytes);
  char* o = (char*)out;
  for (int i = 0; i < n_layers; ++i) {
    const sumk_tf_layer_weights& W = layers[i];
    SUMK_ARG(W.in_proj_w && W.out_proj_w && W.lin1_w && W.lin2_w, "transformer_wplanes_build: null weight in layer %d", i);
    char* lb = o + (size_t)i * l.lay_stride;
    SUMK_TRY(split_planes(W.in_proj_w, 3 * (int64_t)D, D, D, n_planes, lb + l.win, stream));
    SUMK_TRY(split_planes(W.out_proj_w, D, D, D, n_planes, lb + l.wo, stream));
    SUMK_TRY(split_planes(W.lin1_w, F, D, D, n_planes, lb + l.w1, stream));
    SUMK_TRY(split_planes(W.lin2_w, D, F, F, n_planes, lb + l.w2, stream));
  }
  SUMK_ARG(head->k1_w, "transformer_wplanes_build: null k1 weight");
  SUMK_TRY(split_planes(head->k1_w, D, D, D, n_planes, o + l.k1, stream));
  return SUMK_OK;
}

// The one forward: the layer loop of every scoring and training entry.  The plan says which attention core a layer runs (dense; stream in
// exact fp32 or bf16x3, in its scoring or its training form) and whether the projections run on the plane path.
static int tf_forward_any(const char* what, int attn, int32_t training, int attn_prec, float* x, int32_t D, int32_t F, int32_t n_heads,
                          int32_t n_layers, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                          const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head, const sumk_tf_opts* opts,
                          const float* pos_table, const int32_t* pos_rows, float* scores, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(x && seq_off_dev && layers && head && opts && scores && workspace, "%s: null pointer", what);
  SUMK_ARG((pos_table == nullptr) == (pos_rows == nullptr), "%s: pos_table and pos_rows go together", what);
  SUMK_ARG(head->ln_w && head->ln_b && head->k1_w && head->k1_b && head->k2_w && head->k2_b, "%s: null head weight", what);
  for (int l = 0; l < n_layers; ++l) {
    const sumk_tf_layer_weights& W = layers[l];
    SUMK_ARG(W.in_proj_w && W.in_proj_b && W.out_proj_w && W.out_proj_b && W.lin1_w && W.lin1_b && W.lin2_w && W.lin2_b &&
             W.norm1_w && W.norm1_b && W.norm2_w && W.norm2_b, "%s: null weight in layer %d", what, l);
  }
  TfPlan P;
  SUMK_TRY(tf_plan(what, attn, training, attn_prec, D, F, n_heads, n_layers, n_seq, seq_off_host, opts, &P));
  if (workspace_bytes < P.total) {
    set_error(P.planes ? "%s: workspace %zu < %zu the plane path needs (sumk_transformer_workspace_bytes_for)" : "%s: workspace %zu < required %zu",
              what, workspace_bytes, P.total);
    return SUMK_ERR_WORKSPACE;
  }
  const TfGeom& G = P.G; const TfWs& L = G.L; const TfPwExtra& PX = P.px;
  char* ws = (char*)workspace;
  const int R = G.R, dh = G.dh;
  // the plane path: inference in a split-bf16 arithmetic with the weights' planes at hand
  const int npl = P.planes; const bool pw = npl != 0, pw_attn = pw && PX.attn;
  TfWPlanes WL{};
  if (pw) {
    WL = tf_wplanes_layout(D, F, n_layers, npl);
    SUMK_ARG(((uintptr_t)opts->wplanes & 255) == 0, "%s: wplanes must be 256-byte aligned", what);
  }
  char* const PA = ws + PX.pa; char* const PB = ws + PX.pb;
  SeqInfo* const seqinfo = (SeqInfo*)(ws + PX.seqinfo);
  if (pw_attn) {
    hipLaunchKernelGGL(tf_seqinfo_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, seq_off_dev, n_seq, seqinfo);
    // (the slack a V read past the LAST sub-array's pitch lands in: cleared once per call, no kernel writes it -- 0 x stale NaN bits would be NaN)
    SUMK_HIP(hipMemsetAsync(ws + PX.qp + pw_planes_bytes(R, 3 * D, npl) - 8192, 0, 8192, stream));
  }
  const char* const wpl = (const char*)opts->wplanes;
  // C (R, N) = A planes (R, K) x weight planes (N, K)^T + bias [+ Rs] [ReLU]; O: the result as planes instead
  auto pw_linear = [&](const void* Ap, const char* Wp, int N, int K, const float* bias, const float* Rs, int relu, float* C_, void* O_) {
    PwLaunch g; g.A = Ap; g.B = Wp; g.a_rows = R; g.b_rows = N; g.M = R; g.N = N; g.K = K; g.np = npl;
    g.bias = bias; g.R = Rs; g.ldr = N; g.relu = relu; g.C = C_; g.ldc = N; g.O = O_; g.o_rows = R;
    return launch_gemm_pw(O_ ? PW_PLANES : Rs ? PW_RES_F32 : PW_F32, g, stream);
  };
  GemmProb* tabs = (GemmProb*)(ws + L.prob_tabs);
  float* T1 = (float*)(ws + L.t1);
  const Drop dl = make_drop(opts->layer_dropout_p, opts->seed), dhd = make_drop(opts->head_dropout_p, opts->seed);
  const float att_scale = 1.0f / sqrtf((float)dh);
  const TfRun run{&G, ws, D, F, n_heads, n_seq, seq_off_dev, opts->precision, stream, seq_off_host, &P};

  if (pos_table) SUMK_TRY(launch_add_pos(x, pos_table, pos_rows, R, D, stream));
  SUMK_TRY(tf_tables(G, D, F, n_heads, n_seq, seq_off_dev, ws, stream, !P.stream));

  const float* hin = x;
  for (int l = 0; l < n_layers; ++l) {
    const sumk_tf_layer_weights& W = layers[l];
    float *QKV, *E = nullptr, *E2 = nullptr, *CTX, *T1a, *hmid, *FF, *T1b, *hout, *stats = nullptr, *astats = nullptr;
    if (training) {
      char* lb = ws + L.lay0 + (size_t)l * L.lay_stride;
      QKV = (float*)(lb + L.l_qkv);
      if (P.stream) astats = (float*)(lb + L.l_astats);
      else { E = (float*)(lb + L.l_p); E2 = dl.thr ? (float*)(lb + L.l_pd) : nullptr; }
      CTX = (float*)(lb + L.l_ctx); T1a = (float*)(lb + L.l_t1a); hmid = (float*)(lb + L.l_hmid); FF = (float*)(lb + L.l_ff);
      T1b = (float*)(lb + L.l_t1b); hout = (float*)(lb + L.l_hout); stats = (float*)(lb + L.l_stats);
    } else {
      float* Hb[3] = {(float*)(ws + L.h0), (float*)(ws + L.h1), (float*)(ws + L.h2)};
      QKV = (float*)(ws + L.qkv); E = (float*)(ws + L.e); CTX = (float*)(ws + L.ctx); FF = (float*)(ws + L.ff);
      T1a = T1b = T1; hmid = Hb[0]; hout = Hb[1 + (l & 1)];   // never aliases this layer's input (x or the previous hout)
    }
    const uint32_t site = 10u * (uint32_t)l;
    const char* const wl = pw ? wpl + (size_t)l * WL.lay_stride : nullptr;
    if (pw_attn) {   // in-projection -> planes of [Q | K | V] (+ bias); per (video, head): logits + softmax -> alpha planes, alpha . V -> context planes
      SUMK_TRY(split_planes(hin, R, D, D, npl, PA, stream));
      {
        PwLaunch g; g.A = PA; g.B = wl + WL.win; g.a_rows = R; g.b_rows = 3 * (int64_t)D; g.M = R; g.N = 3 * D; g.K = D; g.np = npl;
        g.bias = W.in_proj_b; g.O = ws + PX.qp; g.o_rows = R; g.o_store_rows = pw_rows_pitch(R);      // (pad rows = the bias: finite -- the context kernel multiplies V rows up to 31 past the last video by alpha = 0)
        SUMK_TRY(launch_gemm_pw(PW_PLANES, g, stream));
      }
      SUMK_TRY(launch_attn_pw_logits(npl, ws + PX.qp, R, D, nullptr, ws + PX.ap, seqinfo, n_seq, PX.t_max, att_scale, 0, -1, stream, n_heads));
      SUMK_TRY(launch_attn_pw_context(npl, ws + PX.qp, R, D, ws + PX.ap, PA, seqinfo, n_seq, PX.t_max, stream, n_heads));      // PA: the planes of hin are spent
      SUMK_TRY(pw_linear(PA, wl + WL.wo, D, D, W.out_proj_b, hin, 0, T1a, nullptr));
    } else if (pw) {   // the per-(video, head) products stay on the in-loop kernels (fp32 Q / K / V, logits, context), between plane GEMMs
      SUMK_TRY(split_planes(hin, R, D, D, npl, PA, stream));
      SUMK_TRY(pw_linear(PA, wl + WL.win, 3 * D, D, W.in_proj_b, nullptr, 0, QKV, nullptr));
      SUMK_TRY(tf_attn_core_fwd(run, tabs, QKV, QKV, E, E2, CTX, dl, site + 0));
      SUMK_TRY(split_planes(CTX, R, D, D, npl, PA, stream));
      SUMK_TRY(pw_linear(PA, wl + WL.wo, D, D, W.out_proj_b, hin, 0, T1a, nullptr));
    } else {   // in-projection, the plan's attention core (dense: logits, softmax, context; stream: one launch, no logits), out-projection
      SUMK_TRY(tf_sa_fwd(run, TfAttnW{W.in_proj_w, W.in_proj_b, W.out_proj_w, W.out_proj_b}, hin, QKV, E, E2, CTX, T1a, dl, site, astats));
    }
    SUMK_TRY(launch_layernorm(T1a, hmid, W.norm1_w, W.norm1_b, R, D, opts->layer_eps, stats, stream));
    if (pw) {  // both feed-forward layers; ReLU(lin1) exists as planes only
      SUMK_TRY(split_planes(hmid, R, D, D, npl, PA, stream));
      SUMK_TRY(pw_linear(PA, wl + WL.w1, F, D, W.lin1_b, nullptr, 1, nullptr, PB));
      SUMK_TRY(pw_linear(PB, wl + WL.w2, D, F, W.lin2_b, hmid, 0, T1b, nullptr));
    } else {   // feed-forward 1: bias + ReLU (+dropout); feed-forward 2: bias (+dropout2) + residual
      SUMK_TRY(tf_ff_fwd(run, TfFfW{W.lin1_w, W.lin1_b, W.lin2_w, W.lin2_b}, hmid, FF, T1b, dl, site + 2, site + 3));
    }
    SUMK_TRY(launch_layernorm(T1b, hout, W.norm2_w, W.norm2_b, R, D, opts->layer_eps, stats ? stats + 2 * (size_t)R : nullptr, stream));
    hin = hout;
  }
  float* hfin = training ? (float*)(ws + L.hfin) : (float*)(ws + L.h0);
  float* Z = training ? (float*)(ws + L.z) : T1;
  float* sfin = training ? (float*)(ws + L.stats_fin) : nullptr;
  SUMK_TRY(tf_tail(run, x, hin, hfin, Z, sfin, head, opts, dhd, scores, pw, [&]() -> int {
    SUMK_TRY(split_planes(hfin, R, D, D, npl, PA, stream));
    return pw_linear(PA, wpl + WL.k1, D, D, head->k1_b, nullptr, 1, Z, nullptr);
  }));
  if (training) SUMK_HIP(hipMemcpyAsync(ws + L.scores, scores, (size_t)R * 4, hipMemcpyDeviceToDevice, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

// ---- the forward entries: each names its path to the plan
#define TF_FWD_ARGS x, D, F, n_heads, n_layers, n_seq, seq_off_host, seq_off_dev, layers, head, opts, pos_table, pos_rows, scores, workspace, workspace_bytes, stream_
extern "C" int sumk_transformer_forward(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                        const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                        const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                        const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows,
                                        float* scores, void* workspace, size_t workspace_bytes, int32_t training,
                                        void* stream_) {
  return tf_forward_any("transformer_forward", TF_DENSE, training != 0, 0, TF_FWD_ARGS);
}

extern "C" int sumk_transformer_forward_stream(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                               const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                               const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                               const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows,
                                               float* scores, void* workspace, size_t workspace_bytes, void* stream_) {
  return tf_forward_any("transformer_forward_stream", TF_STREAM, 0, 0, TF_FWD_ARGS);
}

extern "C" int sumk_transformer_forward_stream_split(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                     const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                                     const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                                     const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows,
                                                     float* scores, int32_t attention_precision, void* workspace, size_t workspace_bytes,
                                                     void* stream_) {
  return tf_forward_any("transformer_forward_stream_split", TF_STREAM_SPLIT, 0, attention_precision, TF_FWD_ARGS);
}

extern "C" int sumk_transformer_forward_stream_train(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                     const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                                     const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                                     const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows,
                                                     float* scores, void* workspace, size_t workspace_bytes, void* stream_) {
  return tf_forward_any("transformer_forward_stream_train", TF_STREAM, 1, 0, TF_FWD_ARGS);
}

extern "C" int sumk_transformer_forward_stream_split_train(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                           const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                                           const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                                           const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows,
                                                           float* scores, int32_t attention_precision, void* workspace,
                                                           size_t workspace_bytes, void* stream_) {
  return tf_forward_any("transformer_forward_stream_split_train", TF_STREAM_SPLIT, 1, attention_precision, TF_FWD_ARGS);
}
#undef TF_FWD_ARGS

// The one backward, after a training forward of the same path on the same workspace
static int tf_backward_any(const char* what, int attn, int attn_prec, const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                           int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, const sumk_tf_layer_weights* layers,
                           const sumk_tf_head_weights* head, const sumk_tf_opts* opts, const float* dscores, const sumk_tf_layer_grads* lgr,
                           const sumk_tf_head_grads* hgr, float* dx, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(x && seq_off_dev && layers && head && opts && dscores && lgr && hgr && workspace, "%s: null pointer", what);
  TfPlan P;
  SUMK_TRY(tf_plan(what, attn, 1, attn_prec, D, F, n_heads, n_layers, n_seq, seq_off_host, opts, &P));
  if (workspace_bytes < P.total) {
    set_error("%s: workspace %zu < required %zu (needs the training-mode forward's workspace)", what, workspace_bytes, P.total);
    return SUMK_ERR_WORKSPACE;
  }
  const TfGeom& G = P.G; const TfWs& L = G.L;
  char* ws = (char*)workspace;
  const int R = G.R;
  const int64_t nRD = (int64_t)R * D;
  float* g0 = (float*)(ws + L.g0); float* g1 = (float*)(ws + L.g1); float* g2 = (float*)(ws + L.g2);
  float* dQKV = (float*)(ws + L.dqkv); float* dFF = (float*)(ws + L.dff); float* lnpart = (float*)(ws + L.lnpart);
  const float* hfin = (const float*)(ws + L.hfin); const float* Z = (const float*)(ws + L.z);
  const float* sfin = (const float*)(ws + L.stats_fin); const float* scores = (const float*)(ws + L.scores);
  const Drop dl = make_drop(opts->layer_dropout_p, opts->seed), dhd = make_drop(opts->head_dropout_p, opts->seed);
  const Drop none = make_drop(0.f, 0);
  int nw = 0;
  const TfRun run{&G, ws, D, F, n_heads, n_seq, seq_off_dev, opts->precision, stream, seq_off_host, &P};

  // ---- scoring head: dZ (ReLU + head dropout masks applied), dk2, db2, shared-LN grads
  SUMK_TRY(launch_ln_head_bwd(D, R, Z, sfin + 2 * (size_t)R, head->ln_w, head->ln_b, head->k2_w, scores, dscores, g0, lnpart, dhd,
                              1000u, &nw, stream));
  SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, hgr->ln_w, hgr->ln_b, hgr->k2_w, hgr->k2_b, hgr->k1_b, stream));   // dk1_b = column sums of g0
  SUMK_TRY(tf_wgrad(run, g0, D, D, hfin, D, D, hgr->k1_w));
  SUMK_TRY(tf_nn(run, g0, head->k1_w, g1, P_DD, EPI_NONE, D));               // dHfin' -> g1
  if (opts->more_residuals && dx) SUMK_HIP(hipMemcpyAsync(dx, g1, (size_t)nRD * 4, hipMemcpyDeviceToDevice, stream));
  // encoder's final (shared) LayerNorm
  const float* hlast = (const float*)(ws + L.lay0 + (size_t)(n_layers - 1) * L.lay_stride + L.l_hout);
  SUMK_TRY(launch_ln_bwd_rows(D, R, hlast, sfin, head->ln_w, head->ln_b, g1, g2, lnpart, none, 0u, &nw, stream));
  SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, hgr->ln_w, hgr->ln_b, nullptr, nullptr, nullptr, stream));
  float* dH = g2;            // gradient w.r.t. the current layer's output
  float* fa = g0; float* fb = g1;   // the two free (R,D) buffers

  for (int l = n_layers - 1; l >= 0; --l) {
    const sumk_tf_layer_weights& W = layers[l];
    const sumk_tf_layer_grads& Gd = lgr[l];
    char* lb = ws + L.lay0 + (size_t)l * L.lay_stride;
    const float* QKV = (const float*)(lb + L.l_qkv);
    const float* Pa = P.stream ? nullptr : (const float*)(lb + L.l_p);
    float* E2 = P.stream ? nullptr : (float*)(lb + L.l_pd);
    const float* astats = P.stream ? (const float*)(lb + L.l_astats) : nullptr;
    const float* CTX = (const float*)(lb + L.l_ctx); const float* T1a = (const float*)(lb + L.l_t1a);
    const float* hmid = (const float*)(lb + L.l_hmid); const float* FFa = (const float*)(lb + L.l_ff);
    const float* T1b = (const float*)(lb + L.l_t1b); const float* stats = (const float*)(lb + L.l_stats);
    const float* hin = l == 0 ? x : (const float*)(ws + L.lay0 + (size_t)(l - 1) * L.lay_stride + L.l_hout);
    const uint32_t site = 10u * (uint32_t)l;
    // norm2
    SUMK_TRY(launch_ln_bwd_rows(D, R, T1b, stats + 2 * (size_t)R, W.norm2_w, W.norm2_b, dH, fa, lnpart, none, 0u, &nw, stream));
    SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, Gd.norm2_w, Gd.norm2_b, nullptr, nullptr, nullptr, stream));
    // fa = dT1b (also the residual gradient into hmid) -> fa = dT1b + the feed-forward path = dHmid
    SUMK_TRY(tf_ff_bwd(run, TfFfW{W.lin1_w, W.lin1_b, W.lin2_w, W.lin2_b}, TfFfG{Gd.lin1_w, Gd.lin1_b, Gd.lin2_w, Gd.lin2_b}, hmid, FFa,
                       fa, fb, dFF, dl, site + 2, site + 3));
    // norm1
    SUMK_TRY(launch_ln_bwd_rows(D, R, T1a, stats, W.norm1_w, W.norm1_b, fa, dH, lnpart, none, 0u, &nw, stream));   // dH buffer reused: dT1a
    SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, Gd.norm1_w, Gd.norm1_b, nullptr, nullptr, nullptr, stream));
    // dT1a (in dH) -> dHin: out-projection (dropout1 mask), the plan's attention core, in-projection backward; fa, fb scratch
    SUMK_TRY(tf_sa_bwd(run, TfAttnW{W.in_proj_w, W.in_proj_b, W.out_proj_w, W.out_proj_b},
                       TfAttnG{Gd.in_proj_w, Gd.in_proj_b, Gd.out_proj_w, Gd.out_proj_b}, hin, QKV, Pa, E2, CTX, dH, fa, fb, dQKV, dl, site, astats));
    // dH (= dT1a buffer) now holds the gradient w.r.t. this layer's input = the previous layer's output
  }
  if (dx) {
    if (opts->more_residuals) {
      int64_t n4 = nRD >> 2;
      hipLaunchKernelGGL(add_rows_kernel, tf_blocks(n4), dim3(256), 0, stream, dx, dH, n4);
    } else {
      SUMK_HIP(hipMemcpyAsync(dx, dH, (size_t)nRD * 4, hipMemcpyDeviceToDevice, stream));
    }
  }
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

// ---- the backward entries
#define TF_BWD_ARGS x, D, F, n_heads, n_layers, n_seq, seq_off_host, seq_off_dev, layers, head, opts, dscores, lgr, hgr, dx, workspace, workspace_bytes, stream_
extern "C" int sumk_transformer_backward(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                                         int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                         const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                         const sumk_tf_opts* opts, const float* dscores, const sumk_tf_layer_grads* lgr,
                                         const sumk_tf_head_grads* hgr, float* dx, void* workspace, size_t workspace_bytes,
                                         void* stream_) {
  return tf_backward_any("transformer_backward", TF_DENSE, 0, TF_BWD_ARGS);
}

extern "C" int sumk_transformer_backward_stream(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                                                int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                                const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                                const sumk_tf_opts* opts, const float* dscores, const sumk_tf_layer_grads* lgr,
                                                const sumk_tf_head_grads* hgr, float* dx, void* workspace, size_t workspace_bytes,
                                                void* stream_) {
  return tf_backward_any("transformer_backward_stream", TF_STREAM, 0, TF_BWD_ARGS);
}

extern "C" int sumk_transformer_backward_stream_split(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                                                      int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                                      const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                                      const sumk_tf_opts* opts, const float* dscores, const sumk_tf_layer_grads* lgr,
                                                      const sumk_tf_head_grads* hgr, float* dx, int32_t attention_precision, void* workspace,
                                                      size_t workspace_bytes, void* stream_) {
  return tf_backward_any("transformer_backward_stream_split", TF_STREAM_SPLIT, attention_precision, TF_BWD_ARGS);
}
#undef TF_BWD_ARGS
