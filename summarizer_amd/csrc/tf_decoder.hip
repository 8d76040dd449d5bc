// Transformer stacks of SumGAN-Att (summarizer/models/sumgan_att.py:20-80) for a packed batch of videos on gfx950, exact fp32:
//   * the encoder stack without the scorer head -- n stock post-norm nn.TransformerEncoderLayer, then an optional final LayerNorm
//     (the selector has one, the autoencoder's encoder has none);
//   * the decoder stack -- n stock post-norm nn.TransformerDecoderLayer: norm1(t + SA(t)), norm2(. + CA(., memory)),
//     norm3(. + FF(.)), ReLU, no masks;
//   * the row scaling x * scores between selector and autoencoder (sumgan_att.py:117).
// Every block is transformer.hip's (tf_internal.h): the same fp32 MFMA GEMMs, per-(video, head) problem tables and softmax kernels.
// Cross-attention runs on that attention core with its own tables: Q from the stream (ld D), K / V from the memory's projection,
// which holds every layer's [K | V] side by side (ld 2 n_layers D) and is computed before the first layer in one grouped launch
// (one B operand per layer, GemmLaunch::n_group; four layers per launch).  Deterministic: fixed-order reductions only.
#include "tf_internal.h"
#include <math.h>
#include <algorithm>

namespace sumk {

// ------------------------------------------------------------------------------------------------ decoder workspace
struct TfdWs {
  TfGeom G;                                           // self-attention / feed-forward saves and the backward scratch of transformer.hip
  size_t cross0, cross_stride, c_q, c_p, c_pd, c_ctx, c_t2a, c_h2, c_stats;   // per layer, cross-attention saves
  size_t kv, ctabs, cprob, total;
  int n_chunks, chunk;                                // memory K / V projection: n_chunks launches of up to `chunk` layers
};
enum { CP_DKV = 0, CP_KV0 = 1 };                      // cprob entries: dMemory GEMM, then one per K / V chunk

static int tfd_layout(int D, int F, int heads, int n_layers, int n_seq, const int32_t* off, TfdWs* w) {
  SUMK_ARG(n_layers > 0, "tf_decoder: n_layers=%d", n_layers);
  SUMK_TRY(tf_geometry(D, F, heads, n_layers, n_seq, off, 1, &w->G));
  const TfWs& L = w->G.L;
  const size_t R = (size_t)L.n_rows;
  size_t p = L.total;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  size_t q = 0;
  auto lt = [&](size_t bytes) { size_t at = q; q += align_up(bytes, 256); return at; };
  w->c_q = lt(R * D * 4); w->c_p = lt((size_t)L.e_elems * 4); w->c_pd = lt((size_t)L.e_elems * 4); w->c_ctx = lt(R * D * 4);
  w->c_t2a = lt(R * D * 4); w->c_h2 = lt(R * D * 4); w->c_stats = lt(R * 2 * 4);
  w->cross_stride = q;
  w->cross0 = take(q * (size_t)n_layers);
  w->kv = take(R * 2 * (size_t)D * n_layers * 4);
  w->ctabs = take((size_t)TT_COUNT * n_seq * heads * sizeof(GemmProb));
  // one launch may take several layers only when a layer's 2D columns are whole tiles (the GEMM picks B per tile)
  const int N1 = 2 * D, cfg = gemm_tiles(L.n_rows, N1, 0) >= 512 ? 0 : 1;
  w->chunk = N1 % 128 == 0 && N1 % gemm_tile_n(cfg) == 0 ? 4 : 1;
  w->n_chunks = (n_layers + w->chunk - 1) / w->chunk;
  w->cprob = take((size_t)(CP_KV0 + w->n_chunks) * sizeof(GemmProb));
  w->total = p;
  return SUMK_OK;
}

// per (video, head) cross-attention sub-problems: Q (ld D), K / V at columns [0, D) / [D, 2D) of a layer's slice of the K / V block
// (ld ldkv), context (ld D), dQ (ld D), dK / dV at columns [0, D) / [D, 2D) of a (R, 2D) scratch
__global__ void tfd_cross_setup_kernel(const int32_t* off, int n_seq, int D, int heads, int ldkv, GemmProb* tabs) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  const int dh = D / heads, bt = 64, tnv = (dh + bt - 1) / bt, np = n_seq * heads;
  int64_t eoff = 0; int ts = 0, tpv = 0;
  for (int q = 0; q < s; ++q) {
    int T = off[q + 1] - off[q], tm = (T + bt - 1) / bt;
    eoff += (int64_t)heads * T * ((T + 3) & ~3); ts += heads * tm * tm; tpv += heads * tm * tnv;
  }
  const int row0 = off[s], T = off[s + 1] - row0, ldE = (T + 3) & ~3, tm = (T + bt - 1) / bt;
  auto put = [&](int tab, int h, int64_t a_off, int64_t b_off, int64_t c_off, int M, int N, int K, int lda, int ldb, int ldc,
                 int tile_start, int tiles_n) {
    GemmProb q;
    q.a_off = a_off; q.b_off = b_off; q.c_off = c_off; q.r_off = 0;
    q.M = M; q.N = N; q.K = K; q.lda = lda; q.ldb = ldb; q.ldc = ldc; q.ldr = 0; q.tile_start = tile_start; q.tiles_n = tiles_n;
    for (int i = 0; i < 7; ++i) q.pad_[i] = 0;
    tabs[(size_t)tab * np + s * heads + h] = q;
  };
  for (int h = 0; h < heads; ++h) {
    const int64_t q0 = (int64_t)row0 * D + h * dh, k0 = (int64_t)row0 * ldkv + h * dh, v0 = k0 + D;
    const int64_t dk0 = (int64_t)row0 * 2 * D + h * dh, dv0 = dk0 + D, eb = eoff + (int64_t)h * T * ldE;
    const int t_s = ts + h * tm * tm, t_pv = tpv + h * tm * tnv;
    put(TT_S, h, q0, k0, eb, T, T, dh, D, ldkv, ldE, t_s, tm);            // E = Q_h K_h^T          (NT)
    put(TT_PV, h, eb, v0, q0, T, dh, T, ldE, ldkv, D, t_pv, tnv);         // C_h = alpha_h V_h      (NN)
    put(TT_DV, h, eb, q0, dv0, T, dh, T, ldE, D, 2 * D, t_pv, tnv);       // dV_h = alpha_h^T dC_h  (TN)
    put(TT_DP, h, q0, v0, eb, T, T, dh, D, ldkv, ldE, t_s, tm);           // dAlpha = dC_h V_h^T    (NT)
    put(TT_DQ, h, eb, k0, q0, T, dh, T, ldE, ldkv, D, t_pv, tnv);         // dQ_h = dS K_h          (NN)
    put(TT_DK, h, eb, q0, dk0, T, dh, T, ldE, D, 2 * D, t_pv, tnv);       // dK_h = dS^T Q_h        (TN)
  }
}

static int tf_stack_opts_ok(const sumk_tf_opts* opts, int training, const char* what) {
  SUMK_ARG(opts->precision == SUMK_PRECISION_FP32 && opts->wplanes == nullptr, "%s: exact fp32 only (precision=%d)", what, opts->precision);
  SUMK_ARG(opts->layer_dropout_p >= 0.f && opts->layer_dropout_p < 1.f, "%s: dropout p=%g", what, opts->layer_dropout_p);
  SUMK_ARG(opts->layer_dropout_p == 0.f || training, "%s: dropout needs training mode", what);
  return SUMK_OK;
}

static TfAttnW sa_w(const sumk_tf_layer_weights& W) { return TfAttnW{W.in_proj_w, W.in_proj_b, W.out_proj_w, W.out_proj_b}; }
static TfFfW ff_w(const sumk_tf_layer_weights& W) { return TfFfW{W.lin1_w, W.lin1_b, W.lin2_w, W.lin2_b}; }

// ------------------------------------------------------------------------------------------------ row scaling
__global__ void row_scale_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ y, int64_t n4, int d4) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float f = s[i / d4];
  float4 a = reinterpret_cast<const float4*>(x)[i];
  a.x *= f; a.y *= f; a.z *= f; a.w *= f;
  reinterpret_cast<float4*>(y)[i] = a;
}
// one wave per row: ds = <x, g> (fixed-order shuffle reduction), dx = s g
__global__ __launch_bounds__(256) void row_scale_bwd_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                            const float* __restrict__ g, float* __restrict__ dx,
                                                            float* __restrict__ ds, int64_t n_rows, int d4) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int lane = threadIdx.x & 63;
  const float4* xr = reinterpret_cast<const float4*>(x) + row * d4;
  const float4* gr = reinterpret_cast<const float4*>(g) + row * d4;
  float4* dxr = dx ? reinterpret_cast<float4*>(dx) + row * d4 : nullptr;
  const float f = s[row];
  float dot = 0.f;
  for (int c = lane; c < d4; c += 64) {
    const float4 a = xr[c], b = gr[c];
    dot += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    if (dxr) dxr[c] = make_float4(f * b.x, f * b.y, f * b.z, f * b.w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
  if (ds && lane == 0) ds[row] = dot;
}

}  // namespace sumk

using namespace sumk;

// ------------------------------------------------------------------------------------------------ encoder stack
extern "C" size_t sumk_tf_encoder_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                  const int32_t* seq_off_host, int32_t training) {
  TfWs w;
  if (n_layers < 1 || tf_carve(D, F, n_heads, n_layers, n_seq, seq_off_host, training, &w) != SUMK_OK) return 0;
  return w.total;
}

extern "C" int sumk_tf_encoder_forward(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                       const int32_t* seq_off_host, const int32_t* seq_off_dev, const sumk_tf_layer_weights* layers,
                                       const float* norm_w, const float* norm_b, const sumk_tf_opts* opts, float* hidden,
                                       void* workspace, size_t workspace_bytes, int32_t training, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(x && seq_off_dev && layers && opts && hidden && workspace, "tf_encoder_forward: null pointer");
  SUMK_ARG(n_layers > 0, "tf_encoder_forward: n_layers=%d", n_layers);
  SUMK_ARG((norm_w == nullptr) == (norm_b == nullptr), "tf_encoder_forward: norm_w and norm_b go together");
  SUMK_TRY(tf_stack_opts_ok(opts, training, "tf_encoder_forward"));
  TfGeom G;
  SUMK_TRY(tf_geometry(D, F, n_heads, n_layers, n_seq, seq_off_host, training, &G));
  const TfWs& L = G.L;
  if (workspace_bytes < L.total) { set_error("tf_encoder_forward: workspace %zu < required %zu", workspace_bytes, L.total); return SUMK_ERR_WORKSPACE; }
  char* ws = (char*)workspace;
  const int R = G.R;
  const Drop dl = make_drop(opts->layer_dropout_p, opts->seed);
  const TfRun run{&G, ws, D, F, n_heads, n_seq, seq_off_dev, opts->precision, stream};
  SUMK_TRY(tf_tables(G, D, F, n_heads, n_seq, seq_off_dev, ws, stream));
  float* T1 = (float*)(ws + L.t1);
  const float* hin = x;
  for (int l = 0; l < n_layers; ++l) {
    const sumk_tf_layer_weights& W = layers[l];
    SUMK_ARG(W.in_proj_w && W.in_proj_b && W.out_proj_w && W.out_proj_b && W.lin1_w && W.lin1_b && W.lin2_w && W.lin2_b &&
             W.norm1_w && W.norm1_b && W.norm2_w && W.norm2_b, "tf_encoder_forward: null weight in layer %d", l);
    float *QKV, *E, *E2, *CTX, *T1a, *hmid, *FF, *T1b, *hout, *stats = nullptr;
    if (training) {   // the layout sumk_transformer_backward reads, so the backward blocks are shared as they are
      char* lb = ws + L.lay0 + (size_t)l * L.lay_stride;
      QKV = (float*)(lb + L.l_qkv); E = (float*)(lb + L.l_p); E2 = (float*)(lb + L.l_pd);
      CTX = (float*)(lb + L.l_ctx); T1a = (float*)(lb + L.l_t1a); hmid = (float*)(lb + L.l_hmid); FF = (float*)(lb + L.l_ff);
      T1b = (float*)(lb + L.l_t1b); hout = (float*)(lb + L.l_hout); stats = (float*)(lb + L.l_stats);
    } else {
      float* Hb[3] = {(float*)(ws + L.h0), (float*)(ws + L.h1), (float*)(ws + L.h2)};
      QKV = (float*)(ws + L.qkv); E = (float*)(ws + L.e); E2 = nullptr; CTX = (float*)(ws + L.ctx); FF = (float*)(ws + L.ff);
      T1a = T1b = T1; hmid = Hb[0]; hout = Hb[1 + (l & 1)];   // never aliases this layer's input (x or the previous hout)
    }
    const uint32_t site = 10u * (uint32_t)l;
    SUMK_TRY(tf_sa_fwd(run, sa_w(W), hin, QKV, E, E2, CTX, T1a, dl, site));
    SUMK_TRY(launch_layernorm(T1a, hmid, W.norm1_w, W.norm1_b, R, D, opts->layer_eps, stats, stream));
    SUMK_TRY(tf_ff_fwd(run, ff_w(W), hmid, FF, T1b, dl, site + 2, site + 3));
    SUMK_TRY(launch_layernorm(T1b, hout, W.norm2_w, W.norm2_b, R, D, opts->layer_eps, stats ? stats + 2 * (size_t)R : nullptr, stream));
    hin = hout;
  }
  if (norm_w) SUMK_TRY(launch_layernorm(hin, hidden, norm_w, norm_b, R, D, opts->final_eps, training ? (float*)(ws + L.stats_fin) : nullptr, stream));
  else SUMK_HIP(hipMemcpyAsync(hidden, hin, (size_t)R * D * 4, hipMemcpyDeviceToDevice, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_tf_encoder_backward(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                        const int32_t* seq_off_host, const int32_t* seq_off_dev, const sumk_tf_layer_weights* layers,
                                        const float* norm_w, const float* norm_b, const sumk_tf_opts* opts, const float* dhidden,
                                        const sumk_tf_layer_grads* lgr, float* dnorm_w, float* dnorm_b, float* dx, void* workspace,
                                        size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(x && seq_off_dev && layers && opts && dhidden && lgr && workspace, "tf_encoder_backward: null pointer");
  SUMK_ARG(!norm_w || (norm_b && dnorm_w && dnorm_b), "tf_encoder_backward: the final norm needs its weights and gradients");
  SUMK_TRY(tf_stack_opts_ok(opts, 1, "tf_encoder_backward"));
  TfGeom G;
  SUMK_TRY(tf_geometry(D, F, n_heads, n_layers, n_seq, seq_off_host, 1, &G));
  const TfWs& L = G.L;
  if (workspace_bytes < L.total) { set_error("tf_encoder_backward: workspace %zu < required %zu (needs the training-mode forward's workspace)", workspace_bytes, L.total); return SUMK_ERR_WORKSPACE; }
  char* ws = (char*)workspace;
  const int R = G.R;
  const int64_t nRD = (int64_t)R * D;
  const Drop dl = make_drop(opts->layer_dropout_p, opts->seed), none = make_drop(0.f, 0);
  const TfRun run{&G, ws, D, F, n_heads, n_seq, seq_off_dev, opts->precision, stream};
  float* g0 = (float*)(ws + L.g0); float* g1 = (float*)(ws + L.g1); float* g2 = (float*)(ws + L.g2);
  float* dQKV = (float*)(ws + L.dqkv); float* dFF = (float*)(ws + L.dff); float* lnpart = (float*)(ws + L.lnpart);
  int nw = 0;
  const float* hlast = (const float*)(ws + L.lay0 + (size_t)(n_layers - 1) * L.lay_stride + L.l_hout);
  if (norm_w) {
    SUMK_TRY(launch_ln_bwd_rows(D, R, hlast, (const float*)(ws + L.stats_fin), norm_w, norm_b, dhidden, g2, lnpart, none, 0u, &nw, stream));
    SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, dnorm_w, dnorm_b, nullptr, nullptr, nullptr, stream));
  } else {
    SUMK_HIP(hipMemcpyAsync(g2, dhidden, (size_t)nRD * 4, hipMemcpyDeviceToDevice, stream));
  }
  float* dH = g2; float* fa = g0; float* fb = g1;
  for (int l = n_layers - 1; l >= 0; --l) {
    const sumk_tf_layer_weights& W = layers[l];
    const sumk_tf_layer_grads& Gd = lgr[l];
    char* lb = ws + L.lay0 + (size_t)l * L.lay_stride;
    const float* stats = (const float*)(lb + L.l_stats);
    const float* hin = l == 0 ? x : (const float*)(ws + L.lay0 + (size_t)(l - 1) * L.lay_stride + L.l_hout);
    const uint32_t site = 10u * (uint32_t)l;
    SUMK_TRY(launch_ln_bwd_rows(D, R, (const float*)(lb + L.l_t1b), stats + 2 * (size_t)R, W.norm2_w, W.norm2_b, dH, fa, lnpart, none, 0u, &nw, stream));
    SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, Gd.norm2_w, Gd.norm2_b, nullptr, nullptr, nullptr, stream));
    SUMK_TRY(tf_ff_bwd(run, ff_w(W), TfFfG{Gd.lin1_w, Gd.lin1_b, Gd.lin2_w, Gd.lin2_b}, (const float*)(lb + L.l_hmid),
                       (const float*)(lb + L.l_ff), fa, fb, dFF, dl, site + 2, site + 3));
    SUMK_TRY(launch_ln_bwd_rows(D, R, (const float*)(lb + L.l_t1a), stats, W.norm1_w, W.norm1_b, fa, dH, lnpart, none, 0u, &nw, stream));
    SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, Gd.norm1_w, Gd.norm1_b, nullptr, nullptr, nullptr, stream));
    SUMK_TRY(tf_sa_bwd(run, sa_w(W), TfAttnG{Gd.in_proj_w, Gd.in_proj_b, Gd.out_proj_w, Gd.out_proj_b}, hin,
                       (const float*)(lb + L.l_qkv), (const float*)(lb + L.l_p), (float*)(lb + L.l_pd), (const float*)(lb + L.l_ctx),
                       dH, fa, fb, dQKV, dl, site));
  }
  if (dx) SUMK_HIP(hipMemcpyAsync(dx, dH, (size_t)nRD * 4, hipMemcpyDeviceToDevice, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

// ------------------------------------------------------------------------------------------------ decoder stack
extern "C" size_t sumk_tf_decoder_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                  const int32_t* seq_off_host) {
  TfdWs w;
  if (tfd_layout(D, F, n_heads, n_layers, n_seq, seq_off_host, &w) != SUMK_OK) return 0;
  return w.total;
}

extern "C" int sumk_tf_decoder_forward(const float* tgt, const float* memory, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                                       int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                       const sumk_tf_dec_layer_weights* layers, const sumk_tf_opts* opts, float* out, void* workspace,
                                       size_t workspace_bytes, int32_t training, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(tgt && memory && seq_off_dev && layers && opts && out && workspace, "tf_decoder_forward: null pointer");
  SUMK_TRY(tf_stack_opts_ok(opts, training, "tf_decoder_forward"));
  TfdWs X;
  SUMK_TRY(tfd_layout(D, F, n_heads, n_layers, n_seq, seq_off_host, &X));
  const TfGeom& G = X.G; const TfWs& L = G.L;
  if (workspace_bytes < X.total) { set_error("tf_decoder_forward: workspace %zu < required %zu", workspace_bytes, X.total); return SUMK_ERR_WORKSPACE; }
  for (int l = 0; l < n_layers; ++l) {
    const sumk_tf_dec_layer_weights& W = layers[l];
    SUMK_ARG(W.sa_in_w && W.sa_in_b && W.sa_out_w && W.sa_out_b && W.ca_in_w && W.ca_in_b && W.ca_out_w && W.ca_out_b && W.lin1_w &&
             W.lin1_b && W.lin2_w && W.lin2_b && W.norm1_w && W.norm1_b && W.norm2_w && W.norm2_b && W.norm3_w && W.norm3_b,
             "tf_decoder_forward: null weight in layer %d", l);
  }
  char* ws = (char*)workspace;
  const int R = G.R, ldkv = 2 * D * n_layers;
  const Drop dl = make_drop(opts->layer_dropout_p, opts->seed);
  const TfRun run{&G, ws, D, F, n_heads, n_seq, seq_off_dev, opts->precision, stream};
  GemmProb* prow = (GemmProb*)(ws + L.prob_row);
  GemmProb* ctabs = (GemmProb*)(ws + X.ctabs);
  GemmProb* cprob = (GemmProb*)(ws + X.cprob);
  float* KV = (float*)(ws + X.kv);
  SUMK_TRY(tf_tables(G, D, F, n_heads, n_seq, seq_off_dev, ws, stream));
  hipLaunchKernelGGL(tfd_cross_setup_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, seq_off_dev, n_seq, D, n_heads, ldkv, ctabs);
  // memory's [K | V] for every layer: KV[:, l*2D + (0..2D)] = memory W_l[D:3D]^T + b_l[D:3D], `chunk` layers per launch
  for (int c = 0; c < X.n_chunks; ++c) {
    const int l0 = c * X.chunk, nl = std::min(X.chunk, n_layers - l0), N = 2 * D * nl;
    const int cfg = gemm_tiles(R, N, 0) >= 512 ? 0 : 1;
    SUMK_TRY(fill_single_prob(cprob + CP_KV0 + c, R, N, D, D, D, ldkv, 0, cfg, stream));
    GemmLaunch g; g.precision = opts->precision;
    g.A = memory; g.C = KV + (size_t)l0 * 2 * D; g.probs = cprob + CP_KV0 + c; g.small_tile = cfg; g.total_tiles = gemm_tiles(R, N, cfg);
    g.n_group = nl > 1 ? 2 * D : 0;
    for (int k = 0; k < nl; ++k) { g.B[k] = layers[l0 + k].ca_in_w + (size_t)D * D; g.bias0[k] = layers[l0 + k].ca_in_b + D; }
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_BIAS2, g, stream));
  }
  const float* hin = tgt;
  for (int l = 0; l < n_layers; ++l) {
    const sumk_tf_dec_layer_weights& W = layers[l];
    char* lb = ws + L.lay0 + (size_t)l * L.lay_stride;
    char* cb = ws + X.cross0 + (size_t)l * X.cross_stride;
    float* stats = (float*)(lb + L.l_stats);
    float* h1 = (float*)(lb + L.l_hmid); float* h2 = (float*)(cb + X.c_h2); float* hout = (float*)(lb + L.l_hout);
    const uint32_t site = 10u * (uint32_t)l;
    // self-attention (sites +0, +1), norm1
    SUMK_TRY(tf_sa_fwd(run, TfAttnW{W.sa_in_w, W.sa_in_b, W.sa_out_w, W.sa_out_b}, hin, (float*)(lb + L.l_qkv), (float*)(lb + L.l_p),
                       (float*)(lb + L.l_pd), (float*)(lb + L.l_ctx), (float*)(lb + L.l_t1a), dl, site));
    SUMK_TRY(launch_layernorm((const float*)(lb + L.l_t1a), h1, W.norm1_w, W.norm1_b, R, D, opts->layer_eps, stats, stream));
    // cross-attention (sites +4: weights, +5: dropout2), norm2
    {
      GemmLaunch g; g.precision = opts->precision;   // Q = h1 Wq^T + bq   (rows [0, D) of multihead_attn.in_proj)
      g.A = h1; g.B[0] = W.ca_in_w; g.bias0[0] = W.ca_in_b; g.C = (float*)(cb + X.c_q); g.probs = prow + P_DD; g.small_tile = G.c_dd;
      g.total_tiles = gemm_tiles(R, D, G.c_dd); g.xcd_M = R; g.xcd_N = D; g.lean = gemm_lean_ok(R, D, D, D, D);
      SUMK_TRY(launch_gemm(GEMM_NT, EPI_BIAS2, g, stream));
    }
    SUMK_TRY(tf_attn_core_fwd(run, ctabs, (const float*)(cb + X.c_q), KV + (size_t)l * 2 * D, (float*)(cb + X.c_p), (float*)(cb + X.c_pd),
                              (float*)(cb + X.c_ctx), dl, site + 4));
    SUMK_TRY(tf_out_proj(run, (const float*)(cb + X.c_ctx), W.ca_out_w, W.ca_out_b, h1, (float*)(cb + X.c_t2a), dl, site + 5));
    SUMK_TRY(launch_layernorm((const float*)(cb + X.c_t2a), h2, W.norm2_w, W.norm2_b, R, D, opts->layer_eps, (float*)(cb + X.c_stats), stream));
    // feed-forward (sites +2: after ReLU, +3: dropout3), norm3
    SUMK_TRY(tf_ff_fwd(run, TfFfW{W.lin1_w, W.lin1_b, W.lin2_w, W.lin2_b}, h2, (float*)(lb + L.l_ff), (float*)(lb + L.l_t1b), dl, site + 2, site + 3));
    SUMK_TRY(launch_layernorm((const float*)(lb + L.l_t1b), hout, W.norm3_w, W.norm3_b, R, D, opts->layer_eps, stats + 2 * (size_t)R, stream));
    hin = hout;
  }
  SUMK_HIP(hipMemcpyAsync(out, hin, (size_t)R * D * 4, hipMemcpyDeviceToDevice, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_tf_decoder_backward(const float* tgt, const float* memory, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                                        int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                        const sumk_tf_dec_layer_weights* layers, const sumk_tf_opts* opts, const float* dout,
                                        const sumk_tf_dec_layer_grads* lgr, float* dtgt, float* dmemory, void* workspace,
                                        size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(tgt && memory && seq_off_dev && layers && opts && dout && lgr && workspace, "tf_decoder_backward: null pointer");
  SUMK_TRY(tf_stack_opts_ok(opts, 1, "tf_decoder_backward"));
  TfdWs X;
  SUMK_TRY(tfd_layout(D, F, n_heads, n_layers, n_seq, seq_off_host, &X));
  const TfGeom& G = X.G; const TfWs& L = G.L;
  if (workspace_bytes < X.total) { set_error("tf_decoder_backward: workspace %zu < required %zu (needs the forward's workspace)", workspace_bytes, X.total); return SUMK_ERR_WORKSPACE; }
  char* ws = (char*)workspace;
  const int R = G.R;
  const int64_t nRD = (int64_t)R * D;
  const Drop dl = make_drop(opts->layer_dropout_p, opts->seed), none = make_drop(0.f, 0);
  const TfRun run{&G, ws, D, F, n_heads, n_seq, seq_off_dev, opts->precision, stream};
  GemmProb* cprob = (GemmProb*)(ws + X.cprob);
  const GemmProb* ctabs = (const GemmProb*)(ws + X.ctabs);
  const float* KV = (const float*)(ws + X.kv);
  float* g0 = (float*)(ws + L.g0); float* g1 = (float*)(ws + L.g1); float* g2 = (float*)(ws + L.g2);
  float* dQKV = (float*)(ws + L.dqkv); float* dFF = (float*)(ws + L.dff); float* lnpart = (float*)(ws + L.lnpart);
  float* colpart = (float*)(ws + L.colpart);
  float* dQ = dQKV; float* dKV = dQKV + nRD;          // cross-attention: dQ (R,D), dK | dV (R,2D)
  SUMK_TRY(fill_single_prob(cprob + CP_DKV, R, D, 2 * D, 2 * D, D, D, 0, G.c_dd, stream));   // (R,D) <- (R,2D) x (2D,D)  (NN)
  int nw = 0;
  SUMK_HIP(hipMemcpyAsync(g2, dout, (size_t)nRD * 4, hipMemcpyDeviceToDevice, stream));
  float* dH = g2; float* fa = g0; float* fb = g1;
  bool dmem_started = false;
  for (int l = n_layers - 1; l >= 0; --l) {
    const sumk_tf_dec_layer_weights& W = layers[l];
    const sumk_tf_dec_layer_grads& Gd = lgr[l];
    char* lb = ws + L.lay0 + (size_t)l * L.lay_stride;
    char* cb = ws + X.cross0 + (size_t)l * X.cross_stride;
    const float* stats = (const float*)(lb + L.l_stats);
    const float* h1 = (const float*)(lb + L.l_hmid); const float* h2 = (const float*)(cb + X.c_h2);
    const float* hin = l == 0 ? tgt : (const float*)(ws + L.lay0 + (size_t)(l - 1) * L.lay_stride + L.l_hout);
    const uint32_t site = 10u * (uint32_t)l;
    // norm3, feed-forward: dH -> fa = d h2
    SUMK_TRY(launch_ln_bwd_rows(D, R, (const float*)(lb + L.l_t1b), stats + 2 * (size_t)R, W.norm3_w, W.norm3_b, dH, fa, lnpart, none, 0u, &nw, stream));
    SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, Gd.norm3_w, Gd.norm3_b, nullptr, nullptr, nullptr, stream));
    SUMK_TRY(tf_ff_bwd(run, TfFfW{W.lin1_w, W.lin1_b, W.lin2_w, W.lin2_b}, TfFfG{Gd.lin1_w, Gd.lin1_b, Gd.lin2_w, Gd.lin2_b}, h2,
                       (const float*)(lb + L.l_ff), fa, fb, dFF, dl, site + 2, site + 3));
    // norm2: fa -> dH = dT2a
    SUMK_TRY(launch_ln_bwd_rows(D, R, (const float*)(cb + X.c_t2a), (const float*)(cb + X.c_stats), W.norm2_w, W.norm2_b, fa, dH, lnpart, none, 0u, &nw, stream));
    SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, Gd.norm2_w, Gd.norm2_b, nullptr, nullptr, nullptr, stream));
    // cross-attention: dH -> dH = d h1 (residual + the Q path); dmemory gets the K / V path
    {
      const float* dAO = dH;
      if (dl.thr) { hipLaunchKernelGGL(mask_scale_kernel, dim3((unsigned)((nRD + 255) / 256)), dim3(256), 0, stream, fb, dH, nRD, dl, site + 5); dAO = fb; }
      SUMK_TRY(colsum_accum(dAO, D, R, D, colpart, TF_COLSUM_CHUNKS, Gd.ca_out_b, stream));
      SUMK_TRY(tf_wgrad(run, dAO, D, D, (const float*)(cb + X.c_ctx), D, D, Gd.ca_out_w));
      SUMK_TRY(tf_nn(run, dAO, W.ca_out_w, fa, P_DD, EPI_NONE, D));                                    // fa = dCTX
      SUMK_TRY(tf_attn_core_bwd(run, ctabs, (const float*)(cb + X.c_q), KV + (size_t)l * 2 * D, (const float*)(cb + X.c_p),
                                (float*)(cb + X.c_pd), fa, dQ, dKV, dl, site + 4));
      SUMK_TRY(colsum_accum(dQ, D, R, D, colpart, TF_COLSUM_CHUNKS, Gd.ca_in_b, stream));
      SUMK_TRY(colsum_accum(dKV, 2 * D, R, 2 * D, colpart, TF_COLSUM_CHUNKS, Gd.ca_in_b + D, stream));
      SUMK_TRY(tf_wgrad(run, dQ, D, D, h1, D, D, Gd.ca_in_w));
      SUMK_TRY(tf_wgrad(run, dKV, 2 * D, 2 * D, memory, D, D, Gd.ca_in_w + (size_t)D * D));
      SUMK_TRY(tf_nn(run, dQ, W.ca_in_w, dH, P_DD, EPI_ACCUM, D));                                     // d h1 = dT2a + dQ . Wq
      if (dmemory) {                                                                                   // dmemory (+)= dKV . W[D:3D]
        GemmLaunch g; g.precision = opts->precision;
        g.A = dKV; g.B[0] = W.ca_in_w + (size_t)D * D; g.C = dmemory; g.probs = cprob + CP_DKV; g.small_tile = G.c_dd;
        g.total_tiles = gemm_tiles(R, D, G.c_dd);
        SUMK_TRY(launch_gemm(GEMM_NN, dmem_started ? EPI_ACCUM : EPI_NONE, g, stream));
        dmem_started = true;
      }
    }
    // norm1: dH -> fa = dT1a; self-attention: fa -> fa = d hin
    SUMK_TRY(launch_ln_bwd_rows(D, R, (const float*)(lb + L.l_t1a), stats, W.norm1_w, W.norm1_b, dH, fa, lnpart, none, 0u, &nw, stream));
    SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, Gd.norm1_w, Gd.norm1_b, nullptr, nullptr, nullptr, stream));
    SUMK_TRY(tf_sa_bwd(run, TfAttnW{W.sa_in_w, W.sa_in_b, W.sa_out_w, W.sa_out_b}, TfAttnG{Gd.sa_in_w, Gd.sa_in_b, Gd.sa_out_w, Gd.sa_out_b},
                       hin, (const float*)(lb + L.l_qkv), (const float*)(lb + L.l_p), (float*)(lb + L.l_pd), (const float*)(lb + L.l_ctx),
                       fa, dH, fb, dQKV, dl, site));
    std::swap(dH, fa);
  }
  if (dtgt) SUMK_HIP(hipMemcpyAsync(dtgt, dH, (size_t)nRD * 4, hipMemcpyDeviceToDevice, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

// ------------------------------------------------------------------------------------------------ row scaling
extern "C" int sumk_row_scale_forward(const float* x, const float* s, int64_t n_rows, int32_t D, float* y, void* stream_) {
  SUMK_ARG(x && s && y, "row_scale_forward: null pointer");
  SUMK_ARG(n_rows >= 0 && D > 0 && D % 4 == 0, "row_scale_forward: n_rows=%lld D=%d (D %% 4 == 0)", (long long)n_rows, D);
  const int64_t n4 = n_rows * (D / 4);
  if (n4 == 0) return SUMK_OK;
  hipLaunchKernelGGL(row_scale_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, x, s, y, n4, D / 4);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_row_scale_backward(const float* x, const float* s, const float* g, int64_t n_rows, int32_t D, float* dx, float* ds,
                                       void* stream_) {
  SUMK_ARG(x && s && g, "row_scale_backward: null pointer");
  SUMK_ARG(n_rows >= 0 && D > 0 && D % 4 == 0, "row_scale_backward: n_rows=%lld D=%d (D %% 4 == 0)", (long long)n_rows, D);
  if (n_rows == 0 || (!dx && !ds)) return SUMK_OK;
  hipLaunchKernelGGL(row_scale_bwd_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, x, s, g, dx, ds,
                     n_rows, D / 4);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
