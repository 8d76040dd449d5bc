// Training on the band: the attention of attn_band.hip with what its backward needs kept, and that backward, in O(T w) per video.
// Storage is the forward's (attn_band_common.h): strips of 64 query rows, one 64 x (k_hi - k_lo) rectangle per strip.  A training call keeps
// THREE rectangle buffers of the forward's size:
//   E   alpha
//   E2  dropout(alpha) on the way forward (p > 0 only); dAlphaD, then dLogits, on the way back
//   ET  scratch for TRANSPOSED rectangles
//
// Transposed rectangles.  dV = alphaD^T dCTX and dK = dLogits^T Q contract over the QUERY rows that see a key.  The band is symmetric: key
// strip c (keys 64 c .. 64 c + 63) is seen by exactly the query rows q_lo = ab_k_lo(w, c) .. q_hi = ab_k_hi(T, w, c) -- the same functions,
// hence the same count, pitch and e_off as strip c's own rectangle.  ET therefore has the forward's geometry, entry (key j, row i) at
// e_off_c + (j - 64 c) pitch + (i - q_lo), and with ET filled both products are the forward's CONTEXT launch again: one grouped NN launch of
// the lean kernel, a problem per strip, M = keys of the strip, N = D, K = q_hi - q_lo exactly, A = the transposed rectangle, B = dCTX (Q)
// rows from q_lo.  No split over strips, no atomics, one thread and one order per element.
//
// Launches of the backward, given dCTX (the call only enqueues them):
//   setup      the two setup kernels of the forward, writing the four problem tables below
//   1 transpose(alphaD) -> ET          2 dV = ET dCTX (grouped NN)
//   3 dAlphaD = dCTX V^T -> E2 (the logits launch with A = dCTX, B = V)
//   4 softmax backward in place on E2  5 dQ = dLogits K (grouped NN over exactly the strip's keys)
//   6 transpose(dLogits) -> ET         7 dK = ET Q (grouped NN)
// ET serves both transposes by stream order.  Pad columns [n, pitch) of a rectangle and scratch behind the last video never reach a
// multiplier: the lean kernel zeroes everything at k >= K in registers, and the transpose writes columns [0, n) only.
#include "attn_band_common.h"

namespace sumk {

// The forward softmax (attn_band_softmax_kernel: same NR register forms, same operations) that also writes dropout(alpha) to E2.  The mask of
// entry (row, key) is drawn at site 0, index (packed_row << 20) | key_in_video -- the dense kernel's index, so a band model and a dense
// model with one seed draw the same masks.  The 20 key bits are exactly AB_MAX_T (attn_band_common.h).
template <int NR>
__global__ __launch_bounds__(256) void attn_band_softmax_train_kernel(float* __restrict__ E, float* __restrict__ E2, const ABStrip* __restrict__ strips,
                                                                      float scale, int ignore_self, int aperture, Drop drop_in) {
  const Drop drop = drop_resolve(drop_in);
  const ABStrip t = strips[blockIdx.x >> 4];
  const int rl = (blockIdx.x & 15) * 4 + (threadIdx.x >> 6);
  if (rl >= t.rows) return;
  const int lane = threadIdx.x & 63;
  const int i = t.i0 + rl, n = t.n_keys, k_lo = t.k_lo;
  float* e = E + t.e_off + (int64_t)rl * t.pitch;
  float* e2 = (E2 && drop.thr) ? E2 + t.e_off + (int64_t)rl * t.pitch : nullptr;
  const uint64_t row_bits = (uint64_t)(t.row0 + rl) << 20;
  if constexpr (NR > 0) {
    float v[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) { const int c = lane + 64 * r; v[r] = e[c < n ? c : n - 1]; }
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      v[r] = c < n ? masked_logit(v[r], scale, i, k_lo + c, ignore_self, aperture) : -INFINITY;
      m = fmaxf(m, v[r]);
    }
    m = ab_wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      v[r] = c < n ? expf(v[r] - m) : 0.f;
      sum += v[r];
    }
    sum = ab_wave_sum(sum);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      if (c < n) {
        const float p = v[r] / sum;
        e[c] = p;
        if (e2) e2[c] = drop_apply(drop, 0, row_bits | (uint64_t)(k_lo + c), p);
      }
    }
    return;
  }
  float m = -INFINITY;
  for (int c = lane; c < n; c += 64) m = fmaxf(m, masked_logit(e[c], scale, i, k_lo + c, ignore_self, aperture));
  m = ab_wave_max(m);
  float sum = 0.f;
  for (int c = lane; c < n; c += 64) sum += expf(masked_logit(e[c], scale, i, k_lo + c, ignore_self, aperture) - m);
  sum = ab_wave_sum(sum);
  for (int c = lane; c < n; c += 64) {
    const float p = expf(masked_logit(e[c], scale, i, k_lo + c, ignore_self, aperture) - m) / sum;
    e[c] = p;
    if (e2) e2[c] = drop_apply(drop, 0, row_bits | (uint64_t)(k_lo + c), p);
  }
}

// dLogits = scale * alpha * (drop'(dAlphaD) - sum_j drop'(dAlphaD)_j alpha_j), in place on E2; the operation order of
// vasnet_softmax_bwd_kernel.  One wave per row, the forward's grid and NR forms.  A rectangle corner outside the band has alpha = 0 and gives 0.
template <int NR>
__global__ __launch_bounds__(256) void attn_band_softmax_bwd_kernel(const float* __restrict__ E, float* __restrict__ E2, const ABStrip* __restrict__ strips,
                                                                    float scale, Drop drop_in) {
  const Drop drop = drop_resolve(drop_in);
  const ABStrip t = strips[blockIdx.x >> 4];
  const int rl = (blockIdx.x & 15) * 4 + (threadIdx.x >> 6);
  if (rl >= t.rows) return;
  const int lane = threadIdx.x & 63;
  const int n = t.n_keys, k_lo = t.k_lo;
  const float* p = E + t.e_off + (int64_t)rl * t.pitch;
  float* g = E2 + t.e_off + (int64_t)rl * t.pitch;
  const uint64_t row_bits = (uint64_t)(t.row0 + rl) << 20;
  float dot = 0.f;
  if constexpr (NR > 0) {
    float d[NR], pv[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) { const int c = lane + 64 * r; d[r] = g[c < n ? c : n - 1]; pv[r] = p[c < n ? c : n - 1]; }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      if (c < n) {
        if (drop.thr) d[r] = drop_apply(drop, 0, row_bits | (uint64_t)(k_lo + c), d[r]);
        dot += d[r] * pv[r];
      }
    }
    dot = ab_wave_sum(dot);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      if (c < n) g[c] = pv[r] * (d[r] - dot) * scale;
    }
    return;
  }
  for (int c = lane; c < n; c += 64) {
    float d = g[c];
    if (drop.thr) d = drop_apply(drop, 0, row_bits | (uint64_t)(k_lo + c), d);
    dot += d * p[c];
  }
  dot = ab_wave_sum(dot);
  for (int c = lane; c < n; c += 64) {
    float d = g[c];
    if (drop.thr) d = drop_apply(drop, 0, row_bits | (uint64_t)(k_lo + c), d);
    g[c] = p[c] * (d - dot) * scale;
  }
}

// Rectangles -> transposed rectangles.  Block (c, u): key strip c, query rows q_lo + 64 u .. + 63, one 64 x 64 tile through LDS (rows padded
// to 65 words: the transposed read walks a column with an odd stride, one bank per lane).  Reads run along the keys of one query row,
// writes along the query rows of one key: both contiguous.  Row i of the video starts at (video e_off) + i pitch whatever its strip, and
// key j stands at column j - k_lo(strip of i) there.  An entry with |i - j| > w is written as 0 and never read: the row strip of i need
// not contain key j (at w = 1, row 64 c - 1 belongs to strip c - 1, whose rectangle ends at key 64 c + 1).  An in-band entry always lies
// inside the row strip's rectangle.  Only columns [0, q_hi - q_lo) and the strip's own key rows are written.
__global__ __launch_bounds__(256) void attn_band_transpose_kernel(const float* __restrict__ S, float* __restrict__ ET, const ABStrip* __restrict__ strips, int w) {
  __shared__ float tile[64][65];
  const ABStrip t = strips[blockIdx.x];
  const int u0 = 64 * (int)blockIdx.y;
  if (u0 >= t.n_keys) return;                        // (the strip's n_keys is also its number of query rows, see the head of the file)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q_lo = t.k_lo, nq = t.n_keys;
  const int64_t v_off = t.e_off - (int64_t)t.i0 * t.pitch;      // the video's first rectangle
  const int j = t.i0 + lane;
#pragma unroll 4
  for (int il = wv; il < 64; il += 4) {
    const int u = u0 + il;
    float v = 0.f;
    if (u < nq && lane < t.rows) {
      const int i = q_lo + u;
      const int d = i - j;
      if (d <= w && -d <= w) v = S[v_off + (int64_t)i * t.pitch + (j - ab_k_lo(w, i >> 6))];
    }
    tile[il][lane] = v;
  }
  __syncthreads();
  const int u = u0 + lane;
  if (u >= nq) return;
  for (int jl = wv; jl < t.rows; jl += 4) ET[t.e_off + (int64_t)jl * t.pitch + u] = tile[lane][jl];
}

namespace {
int ab_softmax_nr(int keys_max) { return keys_max <= 256 ? 4 : keys_max <= 640 ? 10 : keys_max <= 1024 ? 16 : 0; }

int ab_transpose(const float* S, float* ET, const ABandWs& L, const ABStrip* strip, int tag, hipStream_t stream) {
  prof_begin(tag, stream);
  hipLaunchKernelGGL(attn_band_transpose_kernel, dim3((unsigned)L.strips, (unsigned)((L.keys_max + 63) / 64)), dim3(256), 0, stream, S, ET, strip, L.w);
  prof_end(tag, stream);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
// one grouped lean launch over the strips
int ab_gemm(GemmLayout layout, const float* A, const float* B, float* C, const GemmProb* probs, const ABandWs& L, bool rect_out, int tag, hipStream_t stream) {
  GemmLaunch g;
  g.A = A; g.B[0] = B; g.C = C; g.probs = probs; g.nprob = (int32_t)L.strips; g.small_tile = 1;
  g.total_tiles = (int32_t)(rect_out ? L.tiles_s : L.tiles_c); g.prof_tag = tag;
  return launch_gemm(layout, EPI_NONE, g, stream);
}
GemmProb* ab_tab(const ABandWs& L, char* ws, int k) { return (GemmProb*)(ws + L.prob + (size_t)k * L.prob_stride); }
}  // namespace

// tables 0 / 1 of the workspace: logits and context; 2 .. 5: the backward's
int attn_band_train_launch(const ABandCall& c, const ABandWs& L, char* ws, int t_max, Drop drop, hipStream_t stream) {
  float* E = (float*)(ws + L.e);
  float* E2 = (float*)(ws + L.e + L.e_stride);
  const ABStrip* strip = (const ABStrip*)(ws + L.strip);
  const ABTab tabs[2] = {{ab_tab(L, ws, 0), 1, c.ldq, c.ldk, 0}, {ab_tab(L, ws, 1), 0, 0, c.ldv, c.ldc}};
  SUMK_TRY(ab_launch_setup(L, ws, c.off_dev, c.n_seq, t_max, c.D, tabs, 2, stream));
  SUMK_TRY(ab_gemm(GEMM_NT, c.Q, c.K, E, tabs[0].prob, L, true, SUMK_PROF_GEMM_QKT, stream));
  {
    const dim3 grid((unsigned)(L.strips * 16)), block(256);
#define SUMK_AB_SOFTMAX(NR) hipLaunchKernelGGL(attn_band_softmax_train_kernel<NR>, grid, block, 0, stream, E, E2, strip, c.scale, c.ignore_self, L.w, drop)
    switch (ab_softmax_nr(L.keys_max)) { case 4: SUMK_AB_SOFTMAX(4); break; case 10: SUMK_AB_SOFTMAX(10); break; case 16: SUMK_AB_SOFTMAX(16); break; default: SUMK_AB_SOFTMAX(0); }
#undef SUMK_AB_SOFTMAX
    SUMK_HIP(hipGetLastError());
  }
  return ab_gemm(GEMM_NN, drop.thr ? E2 : E, c.V, c.ctx, tabs[1].prob, L, false, SUMK_PROF_GEMM_PV, stream);
}

int attn_band_bwd_launch(const ABandBwdCall& c, const ABandWs& L, char* ws, int t_max, Drop drop, hipStream_t stream) {
  float* E = (float*)(ws + L.e);
  float* E2 = (float*)(ws + L.e + L.e_stride);
  float* ET = (float*)(ws + L.e + 2 * L.e_stride);
  const ABStrip* strip = (const ABStrip*)(ws + L.strip);
  const ABTab tabs[4] = {{ab_tab(L, ws, 2), 1, c.lddc, c.ldv, 0},      // dAlphaD = dCTX V^T
                         {ab_tab(L, ws, 3), 0, 0, c.lddc, c.lddv},     // dV = alphaD^T dCTX
                         {ab_tab(L, ws, 4), 0, 0, c.ldk, c.lddq},      // dQ = dLogits K
                         {ab_tab(L, ws, 5), 0, 0, c.ldq, c.lddk}};     // dK = dLogits^T Q
  SUMK_TRY(ab_launch_setup(L, ws, c.off_dev, c.n_seq, t_max, c.D, tabs, 4, stream));
  SUMK_TRY(ab_transpose(drop.thr ? E2 : E, ET, L, strip, SUMK_PROF_BAND_BWD_TRANSPOSE_P, stream));                // 1
  SUMK_TRY(ab_gemm(GEMM_NN, ET, c.dctx, c.dV, tabs[1].prob, L, false, SUMK_PROF_BAND_BWD_DV, stream));            // 2
  SUMK_TRY(ab_gemm(GEMM_NT, c.dctx, c.V, E2, tabs[0].prob, L, true, SUMK_PROF_BAND_BWD_DP, stream));              // 3
  {                                                                                                               // 4
    const dim3 grid((unsigned)(L.strips * 16)), block(256);
#define SUMK_AB_SOFTMAX_BWD(NR) hipLaunchKernelGGL(attn_band_softmax_bwd_kernel<NR>, grid, block, 0, stream, (const float*)E, E2, strip, c.scale, drop)
    prof_begin(SUMK_PROF_BAND_BWD_SOFTMAX, stream);
    switch (ab_softmax_nr(L.keys_max)) { case 4: SUMK_AB_SOFTMAX_BWD(4); break; case 10: SUMK_AB_SOFTMAX_BWD(10); break; case 16: SUMK_AB_SOFTMAX_BWD(16); break; default: SUMK_AB_SOFTMAX_BWD(0); }
    prof_end(SUMK_PROF_BAND_BWD_SOFTMAX, stream);
#undef SUMK_AB_SOFTMAX_BWD
    SUMK_HIP(hipGetLastError());
  }
  SUMK_TRY(ab_gemm(GEMM_NN, E2, c.K, c.dQ, tabs[2].prob, L, false, SUMK_PROF_BAND_BWD_DQ, stream));               // 5
  SUMK_TRY(ab_transpose(E2, ET, L, strip, SUMK_PROF_BAND_BWD_TRANSPOSE_S, stream));                               // 6
  return ab_gemm(GEMM_NN, ET, c.Q, c.dK, tabs[3].prob, L, false, SUMK_PROF_BAND_BWD_DK, stream);                  // 7
}

namespace {
constexpr int VB_SPLITK_PROBS = 64;
constexpr int VB_MAX_D = 2048;          // the LayerNorm backward kernel's register forms

Drop vb_drop(float p, uint64_t seed, const uint64_t* seed_dev) { Drop d = make_drop(p, seed); d.seed_dev = seed_dev; return d; }

// workspace of a training step: fourteen (rows x D) activation / gradient blocks ([Q | K | V] and its gradient are three each), the
// LayerNorm statistics, the scores, the LayerNorm backward's slots, the split-K slab and tables, three one-entry problem tables, the band
struct VBTrainWs { size_t qkv, ctx, y0, y1, z, dz, dy1, dy0, dctx, dqkv, stats, scores, lnpart, slab, slab_elems, pskw, prow; ABandWs band; };
int vbt_carve(const char* who, int D, int n_seq, const int32_t* off, int aperture, VBTrainWs* L) {
  ABandWs probe;
  SUMK_TRY(ab_carve(who, D, n_seq, off, aperture, 0, 3, 6, &probe));      // (checks the batch before off[n_seq] is used)
  SUMK_ARG(D <= VB_MAX_D, "%s: D=%d > %d is not supported by the LayerNorm backward kernel", who, D, VB_MAX_D);
  const size_t R = (size_t)off[n_seq];
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  L->qkv = take(R * 3 * D * 4); L->ctx = take(R * D * 4); L->y0 = take(R * D * 4); L->y1 = take(R * D * 4); L->z = take(R * D * 4);
  L->dz = take(R * D * 4); L->dy1 = take(R * D * 4); L->dy0 = take(R * D * 4); L->dctx = take(R * D * 4); L->dqkv = take(R * 3 * D * 4);
  L->stats = take(R * 4 * 4); L->scores = take(R * 4);
  L->lnpart = take((size_t)(LNB_MAX_WAVES / 4) * ln_slot_floats(D) * 4);
  L->slab_elems = (size_t)32 * D * D; L->slab = take(L->slab_elems * 4);
  L->pskw = take((size_t)2 * VB_SPLITK_PROBS * sizeof(GemmProb));
  L->prow = take(3 * sizeof(GemmProb));
  return ab_carve(who, D, n_seq, off, aperture, p, 3, 6, &L->band);
}

int vb_check_opts(const char* who, const sumk_vasnet_opts* opts) {
  SUMK_ARG(opts->precision == SUMK_PRECISION_FP32, "%s: exact fp32 only, got precision %d", who, opts->precision);
  SUMK_ARG(opts->dropout_p >= 0.f && opts->dropout_p < 1.f, "%s: dropout_p=%f out of [0,1)", who, opts->dropout_p);
  return SUMK_OK;
}
int ab_check_p(const char* who, float p) {
  SUMK_ARG(p >= 0.f && p < 1.f, "%s: dropout_p=%f out of [0,1)", who, p);
  return SUMK_OK;
}
struct VBTiles { int st_qkv, st_d, lean_rows; };
VBTiles vb_tiles(int R, int D) {
  VBTiles t;
  t.st_qkv = (D % 128 == 0 && gemm_tiles(R, 3 * D, 0) >= 512) ? 0 : 1; t.st_d = gemm_tiles(R, D, 0) >= 512 ? 0 : 1;
  t.lean_rows = (D % 32 == 0 && (int64_t)R * 3 * D * 4 < ((int64_t)1 << 31)) ? 1 : 0;
  return t;
}
}  // namespace

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_attn_band_train_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t aperture) {
  ABandWs L;
  if (ab_carve("attn_band_train", D, n_seq, seq_off_host, aperture, 0, 3, 6, &L) != SUMK_OK) return 0;
  return L.total;
}

extern "C" int sumk_attn_band_forward_train(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                                            int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                                            int32_t ignore_self, int32_t aperture, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                                            float* ctx, int32_t ldc, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "attn_band_forward_train";
  SUMK_ARG(Q && K && V && ctx && seq_off_dev && workspace, "%s: null pointer", who);
  ABandWs L;
  SUMK_TRY(ab_carve(who, D, n_seq, seq_off_host, aperture, 0, 3, 6, &L));
  const void* const ptrs[5] = {Q, K, V, ctx, workspace};
  const int32_t lds[5] = {ldq, ldk, ldv, ldc, D};
  SUMK_TRY(ab_check_operands(who, D, ptrs, lds, 5));
  SUMK_TRY(ab_check_p(who, dropout_p));
  if (workspace_bytes < L.total) {
    set_error("%s: workspace %zu < required %zu", who, workspace_bytes, L.total);
    return SUMK_ERR_WORKSPACE;
  }
  ABandCall c;
  c.Q = Q; c.K = K; c.V = V; c.ctx = ctx; c.alpha = nullptr; c.ldq = ldq; c.ldk = ldk; c.ldv = ldv; c.ldc = ldc; c.D = D; c.n_seq = n_seq;
  c.off_dev = seq_off_dev; c.scale = scale; c.ignore_self = ignore_self; c.aperture = aperture;
  return attn_band_train_launch(c, L, (char*)workspace, ab_t_max(n_seq, seq_off_host), vb_drop(dropout_p, seed, seed_dev), stream);
}

extern "C" int sumk_attn_band_backward(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, const float* dctx,
                                       int32_t lddc, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                       float scale, int32_t ignore_self, int32_t aperture, float dropout_p, uint64_t seed,
                                       const uint64_t* seed_dev, float* dQ, int32_t lddq, float* dK, int32_t lddk, float* dV, int32_t lddv,
                                       void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "attn_band_backward";
  SUMK_ARG(Q && K && V && dctx && dQ && dK && dV && seq_off_dev && workspace, "%s: null pointer", who);
  ABandWs L;
  SUMK_TRY(ab_carve(who, D, n_seq, seq_off_host, aperture, 0, 3, 6, &L));
  const void* const ptrs[8] = {Q, K, V, dctx, dQ, dK, dV, workspace};
  const int32_t lds[8] = {ldq, ldk, ldv, lddc, lddq, lddk, lddv, D};
  SUMK_TRY(ab_check_operands(who, D, ptrs, lds, 8));
  SUMK_TRY(ab_check_p(who, dropout_p));
  if (workspace_bytes < L.total) {
    set_error("%s: workspace %zu < required %zu (needs the workspace sumk_attn_band_forward_train left)", who, workspace_bytes, L.total);
    return SUMK_ERR_WORKSPACE;
  }
  ABandBwdCall c;
  c.Q = Q; c.K = K; c.V = V; c.dctx = dctx; c.dQ = dQ; c.dK = dK; c.dV = dV; c.ldq = ldq; c.ldk = ldk; c.ldv = ldv; c.lddc = lddc;
  c.lddq = lddq; c.lddk = lddk; c.lddv = lddv; c.D = D; c.n_seq = n_seq; c.off_dev = seq_off_dev; c.scale = scale; c.ignore_self = ignore_self;
  return attn_band_bwd_launch(c, L, (char*)workspace, ab_t_max(n_seq, seq_off_host), vb_drop(dropout_p, seed, seed_dev), stream);
}

extern "C" size_t sumk_vasnet_band_train_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t aperture) {
  VBTrainWs L;
  if (vbt_carve("vasnet_band_train", D, n_seq, seq_off_host, aperture, &L) != SUMK_OK) return 0;
  return L.band.total;
}

extern "C" int sumk_vasnet_forward_band_train(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                              const sumk_vasnet_weights* w, const sumk_vasnet_opts* opts, float* scores, void* workspace,
                                              size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "vasnet_forward_band_train";
  SUMK_ARG(x && seq_off_dev && w && opts && scores && workspace, "%s: null pointer", who);
  SUMK_ARG(w->Wk && w->Wq && w->Wv && w->Wo && w->W1 && w->b1 && w->w2 && w->b2 && w->ln_w && w->ln_b, "%s: null weight", who);
  SUMK_TRY(vb_check_opts(who, opts));
  VBTrainWs L;
  SUMK_TRY(vbt_carve(who, D, n_seq, seq_off_host, opts->aperture, &L));
  SUMK_ARG(((uintptr_t)x | (uintptr_t)workspace) % 16 == 0, "%s: x and the workspace must be 16-byte aligned", who);
  if (workspace_bytes < L.band.total) {
    set_error("%s: workspace %zu < required %zu", who, workspace_bytes, L.band.total);
    return SUMK_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  const int R = L.band.rows;
  float* QKV = (float*)(ws + L.qkv);
  float* CTX = (float*)(ws + L.ctx);
  float* Y0 = (float*)(ws + L.y0);
  float* Y1 = (float*)(ws + L.y1);
  float* Z = (float*)(ws + L.z);
  float* stats = (float*)(ws + L.stats);
  float* sc = (float*)(ws + L.scores);
  GemmProb* prow = (GemmProb*)(ws + L.prow);
  const Drop drop = vb_drop(opts->dropout_p, opts->seed, opts->seed_dev);
  const VBTiles tl = vb_tiles(R, D);
  SUMK_TRY(fill_single_prob(prow + 0, R, 3 * D, D, D, D, 3 * D, 0, tl.st_qkv, stream));
  SUMK_TRY(fill_single_prob(prow + 1, R, D, D, D, D, D, D, tl.st_d, stream));
  {  // 1: [Q | K | V] = x [Wq; Wk; Wv]^T
    GemmLaunch g;
    g.A = x; g.B[0] = w->Wq; g.B[1] = w->Wk; g.B[2] = w->Wv; g.n_group = D; g.C = QKV; g.probs = prow + 0;
    g.small_tile = tl.st_qkv; g.total_tiles = gemm_tiles(R, 3 * D, tl.st_qkv); g.xcd_M = R; g.xcd_N = 3 * D; g.lean = tl.lean_rows;
    g.prof_tag = SUMK_PROF_GEMM_QKV;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_NONE, g, stream));
  }
  {  // 2-4: logits, softmax (+ dropout site 0), context on the band
    ABandCall c;
    c.Q = QKV; c.K = QKV + D; c.V = QKV + 2 * D; c.ctx = CTX; c.alpha = nullptr; c.ldq = c.ldk = c.ldv = 3 * D; c.ldc = D; c.D = D;
    c.n_seq = n_seq; c.off_dev = seq_off_dev; c.scale = opts->scale; c.ignore_self = opts->ignore_self; c.aperture = opts->aperture;
    SUMK_TRY(attn_band_train_launch(c, L.band, ws, ab_t_max(n_seq, seq_off_host), drop, stream));
  }
  {  // 5: output projection + residual
    GemmLaunch g;
    g.A = CTX; g.B[0] = w->Wo; g.C = Y0; g.R = x; g.probs = prow + 1; g.small_tile = tl.st_d; g.total_tiles = gemm_tiles(R, D, tl.st_d);
    g.xcd_M = R; g.xcd_N = D; g.lean = tl.lean_rows; g.prof_tag = SUMK_PROF_GEMM_OPROJ;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_RESIDUAL, g, stream));
  }
  // 6: dropout (site 1) + LayerNorm
  SUMK_TRY(launch_layernorm_drop(Y0, Y1, w->ln_w, w->ln_b, R, D, opts->eps, stats, drop, 1u, stream));
  {  // 7: k1 + bias + ReLU
    GemmLaunch g;
    g.A = Y1; g.B[0] = w->W1; g.bias0[0] = w->b1; g.C = Z; g.probs = prow + 1; g.small_tile = tl.st_d; g.total_tiles = gemm_tiles(R, D, tl.st_d);
    g.xcd_M = R; g.xcd_N = D; g.lean = tl.lean_rows; g.prof_tag = SUMK_PROF_GEMM_K1;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_BIAS_RELU, g, stream));
  }
  // 8: dropout (site 2) + LayerNorm (same weights) + k2 + sigmoid; the backward reads the scores from the workspace
  SUMK_TRY(launch_ln_head_drop(Z, w->ln_w, w->ln_b, w->w2, w->b2, sc, R, D, opts->eps, stats + 2 * (size_t)R, drop, 2u, stream));
  SUMK_HIP(hipMemcpyAsync(scores, sc, (size_t)R * 4, hipMemcpyDeviceToDevice, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

// The stage order of the dense large-batch backward (sumk_vasnet_backward), the attention stages on the band.
extern "C" int sumk_vasnet_backward_band(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                         const sumk_vasnet_weights* w, const sumk_vasnet_opts* opts, const float* dscores,
                                         const sumk_vasnet_grads* gr, float* dx, void* workspace, size_t workspace_bytes, void* stream_,
                                         void* tail_grads_ready_event) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "vasnet_backward_band";
  SUMK_ARG(x && seq_off_dev && w && opts && dscores && gr && workspace, "%s: null pointer", who);
  SUMK_ARG(w->Wk && w->Wq && w->Wv && w->Wo && w->W1 && w->b1 && w->w2 && w->b2 && w->ln_w && w->ln_b, "%s: null weight", who);
  SUMK_ARG(gr->Wk && gr->Wq && gr->Wv && gr->Wo && gr->W1 && gr->b1 && gr->w2 && gr->b2 && gr->ln_w && gr->ln_b, "%s: null gradient target", who);
  SUMK_TRY(vb_check_opts(who, opts));
  VBTrainWs L;
  SUMK_TRY(vbt_carve(who, D, n_seq, seq_off_host, opts->aperture, &L));
  SUMK_ARG(((uintptr_t)x | (uintptr_t)workspace | (uintptr_t)dx) % 16 == 0, "%s: x, dx and the workspace must be 16-byte aligned", who);
  if (workspace_bytes < L.band.total) {
    set_error("%s: workspace %zu < required %zu (needs the workspace sumk_vasnet_forward_band_train left)", who, workspace_bytes, L.band.total);
    return SUMK_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  const int R = L.band.rows;
  float* QKV = (float*)(ws + L.qkv);
  float* CTX = (float*)(ws + L.ctx);
  float* Y0 = (float*)(ws + L.y0);
  float* Y1 = (float*)(ws + L.y1);
  float* Z = (float*)(ws + L.z);
  float* dZ = (float*)(ws + L.dz);
  float* dY1 = (float*)(ws + L.dy1);
  float* dY0 = (float*)(ws + L.dy0);
  float* dCTX = (float*)(ws + L.dctx);
  float* dQKV = (float*)(ws + L.dqkv);
  float* stats = (float*)(ws + L.stats);
  const float* sc = (const float*)(ws + L.scores);
  float* lnpart = (float*)(ws + L.lnpart);
  float* slab = (float*)(ws + L.slab);
  GemmProb* pskw = (GemmProb*)(ws + L.pskw);
  GemmProb* prow = (GemmProb*)(ws + L.prow);
  const Drop drop = vb_drop(opts->dropout_p, opts->seed, opts->seed_dev);
  const VBTiles tl = vb_tiles(R, D);
  int nw = 0;
  SUMK_TRY(fill_single_prob(prow + 1, R, D, D, D, D, D, D, tl.st_d, stream));              // (R, D) = (R, D) x (D, D)
  if (dx) SUMK_TRY(fill_single_prob(prow + 2, R, D, D, 3 * D, D, D, D, tl.st_d, stream));  // dx += dQKV[:, part] W (A has lda 3 D)
  // 8': head + second LayerNorm + dropout + ReLU -> dZ, dw2, db2, dgamma, dbeta; db1 = column sums of dZ, from the same slots
  SUMK_TRY(launch_ln_head_bwd(D, R, Z, stats + 2 * (size_t)R, w->ln_w, w->ln_b, w->w2, sc, dscores, dZ, lnpart, drop, 2u, &nw, stream));
  SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, gr->ln_w, gr->ln_b, gr->w2, gr->b2, gr->b1, stream));
  {  // 7': dY1 = dZ W1
    GemmLaunch g;
    g.A = dZ; g.B[0] = w->W1; g.C = dY1; g.probs = prow + 1; g.small_tile = tl.st_d; g.total_tiles = gemm_tiles(R, D, tl.st_d); g.xcd_M = R; g.xcd_N = D;
    SUMK_TRY(launch_gemm(GEMM_NN, EPI_NONE, g, stream));
  }
  // 6': first LayerNorm + dropout -> dY0
  SUMK_TRY(launch_ln_bwd_rows(D, R, Y0, stats, w->ln_w, w->ln_b, dY1, dY0, lnpart, drop, 1u, &nw, stream));
  SUMK_TRY(ln_bwd_reduce(lnpart, nw, D, gr->ln_w, gr->ln_b, nullptr, nullptr, nullptr, stream));
  {  // 5' + 7': dWo += dY0^T CTX and dW1 += dZ^T Y1 in one split-K launch, then dCTX = dY0 Wo
    const float* const As[2] = {dY0, dZ};
    const float* const Bs[2] = {CTX, Y1};
    float* out[4] = {gr->Wo, gr->W1, nullptr, nullptr};
    SUMK_TRY(gemm_tn_splitk_accum_multi(2, As, Bs, D, D, D, D, R, slab, L.slab_elems, pskw, VB_SPLITK_PROBS, out, D, D, 1.f, stream));
    GemmLaunch g;
    g.A = dY0; g.B[0] = w->Wo; g.C = dCTX; g.probs = prow + 1; g.small_tile = tl.st_d; g.total_tiles = gemm_tiles(R, D, tl.st_d); g.xcd_M = R; g.xcd_N = D;
    SUMK_TRY(launch_gemm(GEMM_NN, EPI_NONE, g, stream));
  }
  // Wo, W1, b1, w2, b2 are final from here on (where the dense backward records the event)
  if (tail_grads_ready_event) SUMK_HIP(hipEventRecord((hipEvent_t)tail_grads_ready_event, stream));
  {  // 4' - 2': the attention backward on the band
    ABandBwdCall c;
    c.Q = QKV; c.K = QKV + D; c.V = QKV + 2 * D; c.dctx = dCTX; c.dQ = dQKV; c.dK = dQKV + D; c.dV = dQKV + 2 * D;
    c.ldq = c.ldk = c.ldv = c.lddq = c.lddk = c.lddv = 3 * D; c.lddc = D; c.D = D; c.n_seq = n_seq; c.off_dev = seq_off_dev;
    c.scale = opts->scale; c.ignore_self = opts->ignore_self;
    SUMK_TRY(attn_band_bwd_launch(c, L.band, ws, ab_t_max(n_seq, seq_off_host), drop, stream));
  }
  {  // 1': d[Wq; Wk; Wv] += dQKV^T x
    float* out[4] = {gr->Wq, gr->Wk, gr->Wv, nullptr};
    SUMK_TRY(gemm_tn_splitk_accum(dQKV, 3 * D, x, D, 3 * D, D, R, slab, L.slab_elems, pskw + VB_SPLITK_PROBS, VB_SPLITK_PROBS, out, D, D, 1.f, stream));
  }
  if (dx) {  // dx = dY0 (residual) + dQ Wq + dK Wk + dV Wv
    SUMK_HIP(hipMemcpyAsync(dx, dY0, (size_t)R * D * 4, hipMemcpyDeviceToDevice, stream));
    const float* Ws[3] = {w->Wq, w->Wk, w->Wv};
    for (int part = 0; part < 3; ++part) {
      GemmLaunch g;
      g.A = dQKV + (size_t)part * D; g.B[0] = Ws[part]; g.C = dx; g.probs = prow + 2; g.small_tile = tl.st_d;
      g.total_tiles = gemm_tiles(R, D, tl.st_d); g.xcd_M = R; g.xcd_N = D;
      SUMK_TRY(launch_gemm(GEMM_NN, EPI_ACCUM, g, stream));
    }
  }
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
