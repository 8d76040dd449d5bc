// Local attention on the band: VASNet's `local` option (aperture w >= 0, vasnet.py:124-127) in O(T w) per video instead of the dense
// path's (T x T) logits block (vasnet.hip) -- the scorer in front of sumk_kts_banded and the long evaluation tail.  Same definition as the
// dense path (masked_logit, sumk_internal.h), exact fp32, inference only.
//
// Storage.  A video of T steps is cut into strips of 64 query rows.  Strip r (rows 64 r .. 64 r + 63) can only see the keys
// k_lo = max(0, 64 r - w) .. k_hi = min(T, 64 r + 64 + w) and keeps a rectangle of 64 x (k_hi - k_lo) fp32 logits: entry (row i, key j)
// at e_off + (i - 64 r) pitch + (j - k_lo), pitch = min(T, 2 w + 64) rounded up to 4.  Rectangles of all strips of all videos lie back to
// back; offsets are int64 elements.  The corners of a rectangle outside |i - j| <= w are computed and masked like every other entry
// (64 / (2 w + 64) of the work at worst); nothing of size T x T exists.
//
// Launches (the call only enqueues them):
//   setup    two small kernels: per video its offsets (sums of aband_sizes over the videos before it, as ab_carve adds them on the host),
//            per strip one GemmProb for the logits, one for the context and the record the softmax reads
//   logits   ONE grouped launch_gemm (NT, 64x64 tiles, EPI_NONE): problem = strip, M = rows of the strip, N = its keys, K = D, A = Q rows,
//            B = K rows from k_lo.  The lean kernel of the dense path's per-video launch, same k order: a logit has the dense path's bits.
//   softmax  in place on the rectangles, one wave per row: masked_logit, max, expf(e - m) / sum; an all-masked row is NaN as in torch
//   context  ONE grouped launch_gemm (NN, EPI_NONE): M = rows, N = D, K = k_hi - k_lo EXACTLY, A = the rectangle, B = V rows from k_lo.
//            The K tail of the lean kernel clamps the row index of B to K - 1 and zeroes what lies behind it in registers, so V rows of
//            the next video, or poisoned scratch behind the last one, never reach a multiplier (0 x NaN = NaN: zero alpha is not enough).
// The grouped kernel takes these tables as they are -- no strip kernel of its own was needed.
// No atomics, no cooperative launch, no flag polled across workgroups; every element is produced by one thread in a fixed order.
#include "attn_band_common.h"

namespace sumk {

int ab_carve(const char* who, int D, int n_seq, const int32_t* off, int aperture, size_t base, int n_e, int n_tab, ABandWs* L) {
  SUMK_ARG(D > 0 && D % 4 == 0, "%s: D=%d must be a positive multiple of 4", who, D);
  SUMK_ARG(n_seq > 0 && n_seq <= 65535 && off && off[0] == 0, "%s: empty batch (or more than 65535 videos)", who);
  SUMK_ARG(aperture >= 0, "%s: the band needs an aperture >= 0, got %d", who, aperture);
  const int w = ab_clamp_w(aperture);
  int64_t e = 0, strips = 0, tiles = 0; int keys_max = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int64_t T = (int64_t)off[s + 1] - off[s];
    SUMK_ARG(T >= 1 && T <= AB_MAX_T, "%s: video %d has %lld steps (1 .. %d supported)", who, s, (long long)T, AB_MAX_T);
    const ABandSizes z = aband_sizes((int)T, w);
    e += z.e; strips += z.strips; tiles += z.tiles_s;
    keys_max = z.pitch > keys_max ? z.pitch : keys_max;
  }
  const int64_t tiles_c = strips * ((D + 63) / 64);
  SUMK_ARG(tiles < ((int64_t)1 << 31) && tiles_c < ((int64_t)1 << 31), "%s: %lld logits / %lld context tiles do not fit one launch",
           who, (long long)tiles, (long long)tiles_c);
  size_t p = base;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  L->e = p; L->e_stride = align_up((size_t)e * 4, 256);
  for (int k = 0; k < n_e; ++k) take((size_t)e * 4);
  L->seq = take((size_t)n_seq * sizeof(ABSeq));
  L->strip = take((size_t)strips * sizeof(ABStrip));
  L->prob = p; L->prob_stride = align_up((size_t)strips * sizeof(GemmProb), 256);
  for (int k = 0; k < n_tab; ++k) take((size_t)strips * sizeof(GemmProb));
  L->total = p; L->e_elems = e; L->strips = strips; L->tiles_s = tiles; L->tiles_c = tiles_c; L->w = w; L->keys_max = keys_max; L->rows = off[n_seq];
  return SUMK_OK;
}

int ab_t_max(int n_seq, const int32_t* off) {
  int t = 0;
  for (int s = 0; s < n_seq; ++s) t = off[s + 1] - off[s] > t ? off[s + 1] - off[s] : t;
  return t;
}

int ab_check_operands(const char* who, int D, const void* const ptrs[], const int32_t lds[], int n) {
  const int ld_max = 1 << 22;      // (a 64-row tile of an operand stays far below the 2^31 bytes the GEMM's 32-bit row offsets span)
  for (int k = 0; k < n; ++k) {
    SUMK_ARG(lds[k] >= D && lds[k] % 4 == 0 && lds[k] <= ld_max, "%s: leading dimensions must be multiples of 4 in D .. %d, got %d", who, ld_max, lds[k]);
    SUMK_ARG((uintptr_t)ptrs[k] % 16 == 0, "%s: pointers must be 16-byte aligned", who);
  }
  return SUMK_OK;
}

// One thread per video: where its rectangles, strips and logits tiles start.
__global__ void attn_band_seq_kernel(const int32_t* off, int n_seq, int w, ABSeq* seq) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  int64_t e = 0, ts = 0; int st = 0;
  for (int q = 0; q < s; ++q) {
    const ABandSizes z = aband_sizes(off[q + 1] - off[q], w);
    e += z.e; ts += z.tiles_s; st += z.strips;
  }
  ABSeq k;
  k.e_off = e; k.tile_s0 = ts; k.row0 = off[s]; k.T = off[s + 1] - off[s]; k.strip0 = st; k.pitch = aband_sizes(k.T, w).pitch;
  seq[s] = k;
}

// One thread per (video, strip): the strip's record and its GEMM problems (ABTab, attn_band_common.h).
__global__ void attn_band_strip_kernel(ABSetup a) {
  const ABSeq v = a.seq[blockIdx.y];
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (v.T + 63) / 64) return;
  const int k_lo = ab_k_lo(a.w, r), n_keys = ab_k_hi(v.T, a.w, r) - k_lo;
  const int rows = v.T - 64 * r < 64 ? v.T - 64 * r : 64;
  const int64_t e_off = v.e_off + (int64_t)r * 64 * v.pitch;
  const int idx = v.strip0 + r;
  ABStrip t;
  t.e_off = e_off; t.row0 = v.row0 + 64 * r; t.rows = rows; t.i0 = 64 * r; t.k_lo = k_lo; t.n_keys = n_keys; t.pitch = v.pitch;
  a.strip[idx] = t;
  GemmProb q;
  for (int i = 0; i < 7; ++i) q.pad_[i] = 0;
  q.r_off = 0; q.ldr = 0;
  for (int k = 0; k < a.n_tab; ++k) {
    const ABTab tb = a.tab[k];
    if (tb.rect_out) {      // C(rows, n_keys) = A[row0 ..] B[k_lo ..]^T into the rectangle
      q.a_off = (int64_t)t.row0 * tb.lda; q.b_off = (int64_t)(v.row0 + k_lo) * tb.ldb; q.c_off = e_off;
      q.M = rows; q.N = n_keys; q.K = a.D; q.lda = tb.lda; q.ldb = tb.ldb; q.ldc = v.pitch;
      q.tiles_n = (n_keys + 63) / 64; q.tile_start = (int32_t)(v.tile_s0 + ab_tiles_before(v.T, a.w, r));
    } else {                // C(rows, D) = rect(rows, n_keys) B[k_lo .. k_lo + n_keys)
      q.a_off = e_off; q.b_off = (int64_t)(v.row0 + k_lo) * tb.ldb; q.c_off = (int64_t)t.row0 * tb.ldc;
      q.M = rows; q.N = a.D; q.K = n_keys; q.lda = v.pitch; q.ldb = tb.ldb; q.ldc = tb.ldc;
      q.tiles_n = (a.D + 63) / 64; q.tile_start = idx * q.tiles_n;
    }
    tb.prob[idx] = q;
  }
}

int ab_launch_setup(const ABandWs& L, char* ws, const int32_t* off_dev, int n_seq, int t_max, int D, const ABTab* tabs, int n_tab, hipStream_t stream) {
  ABSeq* seq = (ABSeq*)(ws + L.seq);
  hipLaunchKernelGGL(attn_band_seq_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, off_dev, n_seq, L.w, seq);
  ABSetup su;
  su.seq = seq; su.strip = (ABStrip*)(ws + L.strip); su.n_tab = n_tab; su.w = L.w; su.D = D;
  for (int k = 0; k < 6; ++k) su.tab[k] = k < n_tab ? tabs[k] : ABTab{nullptr, 0, 0, 0, 0};
  hipLaunchKernelGGL(attn_band_strip_kernel, dim3(((t_max + 63) / 64 + 63) / 64, n_seq), dim3(64), 0, stream, su);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

// Band softmax, in place.  One wave per query row, four rows per block, 16 blocks per strip.  NR > 0: the row (n_keys <= 64 NR) lives in
// registers and every load is issued before the first reduction; NR == 0: any length, three passes over the (L2-resident) row.  Same
// operations per element either way.  alpha (test entry): entry j - (i - w) of the row's 2 w + 1, zeros for keys outside the video.
template <int NR>
__global__ __launch_bounds__(256) void attn_band_softmax_kernel(float* __restrict__ E, const ABStrip* __restrict__ strips, float scale,
                                                                int ignore_self, int aperture, float* __restrict__ alpha) {
  const ABStrip t = strips[blockIdx.x >> 4];
  const int rl = (blockIdx.x & 15) * 4 + (threadIdx.x >> 6);
  if (rl >= t.rows) return;
  const int lane = threadIdx.x & 63;
  const int i = t.i0 + rl, n = t.n_keys, k_lo = t.k_lo;
  float* e = E + t.e_off + (int64_t)rl * t.pitch;
  // alpha row: column of key j is j - i + w.  (aperture <= AB_MAX_T whenever alpha is given: int64 only for the row offset)
  float* arow = alpha ? alpha + (int64_t)(t.row0 + rl) * ((int64_t)2 * aperture + 1) + ((int64_t)aperture - i) : nullptr;
  auto in_band = [&](int j) { return j - i <= aperture && i - j <= aperture; };
  if (arow) {   // keys of the band that lie outside the video: below 0 or at / past T (= behind the last strip's k_hi)
    const int64_t j_end = (int64_t)i + aperture;      // last key of the band
    for (int64_t j = (int64_t)i - aperture + lane; j < 0; j += 64) arow[j] = 0.f;
    // inside the video every in-band key lies in [k_lo, k_lo + n); what is in the band behind k_lo + n is therefore past T
    for (int64_t j = (int64_t)k_lo + n + lane; j <= j_end; j += 64) arow[j] = 0.f;
  }
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
        if (arow && in_band(k_lo + c)) arow[k_lo + c] = p;
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
    if (arow && in_band(k_lo + c)) arow[k_lo + c] = p;
  }
}

// the four launches + setup; every argument has been checked
int attn_band_launch(const ABandCall& c, const ABandWs& L, char* ws, int t_max, hipStream_t stream) {
  float* E = (float*)(ws + L.e);
  ABStrip* strip = (ABStrip*)(ws + L.strip);
  GemmProb* prob_s = (GemmProb*)(ws + L.prob);
  GemmProb* prob_c = (GemmProb*)(ws + L.prob + L.prob_stride);
  const ABTab tabs[2] = {{prob_s, 1, c.ldq, c.ldk, 0}, {prob_c, 0, 0, c.ldv, c.ldc}};
  SUMK_TRY(ab_launch_setup(L, ws, c.off_dev, c.n_seq, t_max, c.D, tabs, 2, stream));
  {
    GemmLaunch g;
    g.A = c.Q; g.B[0] = c.K; g.C = E; g.probs = prob_s; g.nprob = (int32_t)L.strips; g.small_tile = 1; g.total_tiles = (int32_t)L.tiles_s;
    g.prof_tag = SUMK_PROF_GEMM_QKT;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_NONE, g, stream));
  }
  {
    const dim3 grid((unsigned)(L.strips * 16)), block(256);
    // aperture as the kernels see it: the clamped one masks the same entries (no |i - j| reaches it) and keeps j - i + w inside int32
#define SUMK_AB_SOFTMAX(NR) hipLaunchKernelGGL(attn_band_softmax_kernel<NR>, grid, block, 0, stream, E, (const ABStrip*)strip, c.scale, c.ignore_self, L.w, c.alpha)
    prof_begin(SUMK_PROF_BAND_SOFTMAX, stream);
    if (L.keys_max <= 256) SUMK_AB_SOFTMAX(4); else if (L.keys_max <= 640) SUMK_AB_SOFTMAX(10); else if (L.keys_max <= 1024) SUMK_AB_SOFTMAX(16);
    else SUMK_AB_SOFTMAX(0);
    prof_end(SUMK_PROF_BAND_SOFTMAX, stream);
#undef SUMK_AB_SOFTMAX
    SUMK_HIP(hipGetLastError());
  }
  {
    GemmLaunch g;
    g.A = E; g.B[0] = c.V; g.C = c.ctx; g.probs = prob_c; g.nprob = (int32_t)L.strips; g.small_tile = 1; g.total_tiles = (int32_t)L.tiles_c;
    g.prof_tag = SUMK_PROF_GEMM_PV;
    SUMK_TRY(launch_gemm(GEMM_NN, EPI_NONE, g, stream));
  }
  return SUMK_OK;
}

namespace {
// workspace of the forward: [Q | K | V] (rows x 3 D; the first LayerNorm's output takes its place once the context exists), the context (later
// k1's output), the residual sum, three one-entry problem tables, then the band
struct VBandWs { size_t qkv, ctx, y0, prow; ABandWs band; };
int vb_carve(int D, int n_seq, const int32_t* off, int aperture, VBandWs* L) {
  ABandWs probe;
  SUMK_TRY(ab_carve("vasnet_forward_band", D, n_seq, off, aperture, 0, 1, 2, &probe));      // (checks the batch before off[n_seq] is used)
  const size_t rd = align_up((size_t)off[n_seq] * D * 4, 256);
  L->qkv = 0; L->ctx = 3 * rd; L->y0 = 4 * rd; L->prow = 5 * rd;
  return ab_carve("vasnet_forward_band", D, n_seq, off, aperture, 5 * rd + align_up(3 * sizeof(GemmProb), 256), 1, 2, &L->band);
}
}  // namespace

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_attn_band_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t aperture) {
  ABandWs L;
  if (ab_carve("attn_band", D, n_seq, seq_off_host, aperture, 0, 1, 2, &L) != SUMK_OK) return 0;
  return L.total;
}

extern "C" int sumk_attn_band(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D, int32_t n_seq,
                              const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale, int32_t ignore_self, int32_t aperture,
                              float* ctx, int32_t ldc, float* alpha, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(Q && K && V && ctx && seq_off_dev && workspace, "attn_band: null pointer");
  ABandWs L;
  SUMK_TRY(ab_carve("attn_band", D, n_seq, seq_off_host, aperture, 0, 1, 2, &L));
  const int ld_max = 1 << 22;      // (a 64-row tile of an operand stays far below the 2^31 bytes the GEMM's 32-bit row offsets span)
  SUMK_ARG(ldq >= D && ldk >= D && ldv >= D && ldc >= D && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldc % 4 == 0 && ldq <= ld_max &&
           ldk <= ld_max && ldv <= ld_max && ldc <= ld_max, "attn_band: leading dimensions must be multiples of 4 in D .. %d, got %d %d %d %d",
           ld_max, ldq, ldk, ldv, ldc);
  SUMK_ARG(((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)ctx | (uintptr_t)workspace) % 16 == 0, "attn_band: pointers must be 16-byte aligned");
  SUMK_ARG(alpha == nullptr || aperture <= AB_MAX_T, "attn_band: the alpha output needs aperture <= %d", AB_MAX_T);
  if (workspace_bytes < L.total) {
    set_error("attn_band: workspace %zu < required %zu", workspace_bytes, L.total);
    return SUMK_ERR_WORKSPACE;
  }
  ABandCall c;
  c.Q = Q; c.K = K; c.V = V; c.ctx = ctx; c.alpha = alpha; c.ldq = ldq; c.ldk = ldk; c.ldv = ldv; c.ldc = ldc; c.D = D; c.n_seq = n_seq;
  c.off_dev = seq_off_dev; c.scale = scale; c.ignore_self = ignore_self; c.aperture = aperture;
  return attn_band_launch(c, L, (char*)workspace, ab_t_max(n_seq, seq_off_host), stream);
}

extern "C" size_t sumk_vasnet_band_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t aperture) {
  VBandWs L;
  if (vb_carve(D, n_seq, seq_off_host, aperture, &L) != SUMK_OK) return 0;
  return L.band.total;
}

extern "C" int sumk_vasnet_forward_band(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                        const sumk_vasnet_weights* w, const sumk_vasnet_opts* opts, float* scores, void* workspace,
                                        size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(x && seq_off_dev && w && opts && scores && workspace, "vasnet_forward_band: null pointer");
  SUMK_ARG(w->Wk && w->Wq && w->Wv && w->Wo && w->W1 && w->b1 && w->w2 && w->b2 && w->ln_w && w->ln_b, "vasnet_forward_band: null weight");
  SUMK_ARG(opts->precision == SUMK_PRECISION_FP32, "vasnet_forward_band: exact fp32 only, got precision %d", opts->precision);
  SUMK_ARG(opts->dropout_p == 0.f, "vasnet_forward_band: inference only (dropout_p=%f)", opts->dropout_p);
  VBandWs L;
  SUMK_TRY(vb_carve(D, n_seq, seq_off_host, opts->aperture, &L));
  SUMK_ARG(((uintptr_t)x | (uintptr_t)workspace) % 16 == 0, "vasnet_forward_band: x and the workspace must be 16-byte aligned");
  if (workspace_bytes < L.band.total) {
    set_error("vasnet_forward_band: workspace %zu < required %zu", workspace_bytes, L.band.total);
    return SUMK_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  const int R = L.band.rows;
  float* QKV = (float*)(ws + L.qkv);
  float* CTX = (float*)(ws + L.ctx);
  float* Y0 = (float*)(ws + L.y0);
  float* Y1 = QKV;          // [Q | K | V] is dead once the context exists
  float* Z = CTX;           // the context is dead once the output projection has read it
  GemmProb* prow = (GemmProb*)(ws + L.prow);
  // row-wise problems: 128x128 tiles when they fill the chip (and a 128-column tile stays inside one of the three projection matrices)
  const int st_qkv = (D % 128 == 0 && gemm_tiles(R, 3 * D, 0) >= 512) ? 0 : 1, st_d = gemm_tiles(R, D, 0) >= 512 ? 0 : 1;
  const int lean_rows = (D % 32 == 0 && (int64_t)R * 3 * D * 4 < ((int64_t)1 << 31)) ? 1 : 0;
  SUMK_TRY(fill_single_prob(prow + 0, R, 3 * D, D, D, D, 3 * D, 0, st_qkv, stream));
  SUMK_TRY(fill_single_prob(prow + 1, R, D, D, D, D, D, D, st_d, stream));
  {  // 1: [Q | K | V] = x [Wq; Wk; Wv]^T
    GemmLaunch g;
    g.A = x; g.B[0] = w->Wq; g.B[1] = w->Wk; g.B[2] = w->Wv; g.n_group = D; g.C = QKV; g.probs = prow + 0;
    g.small_tile = st_qkv; g.total_tiles = gemm_tiles(R, 3 * D, st_qkv); g.xcd_M = R; g.xcd_N = 3 * D; g.lean = lean_rows;
    g.prof_tag = SUMK_PROF_GEMM_QKV;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_NONE, g, stream));
  }
  {  // 2-4: logits, softmax, context on the band
    ABandCall c;
    c.Q = QKV; c.K = QKV + D; c.V = QKV + 2 * D; c.ctx = CTX; c.alpha = nullptr; c.ldq = c.ldk = c.ldv = 3 * D; c.ldc = D; c.D = D;
    c.n_seq = n_seq; c.off_dev = seq_off_dev; c.scale = opts->scale; c.ignore_self = opts->ignore_self; c.aperture = opts->aperture;
    SUMK_TRY(attn_band_launch(c, L.band, ws, ab_t_max(n_seq, seq_off_host), stream));
  }
  {  // 5: output projection + residual
    GemmLaunch g;
    g.A = CTX; g.B[0] = w->Wo; g.C = Y0; g.R = x; g.probs = prow + 1; g.small_tile = st_d; g.total_tiles = gemm_tiles(R, D, st_d);
    g.xcd_M = R; g.xcd_N = D; g.lean = lean_rows; g.prof_tag = SUMK_PROF_GEMM_OPROJ;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_RESIDUAL, g, stream));
  }
  // 6: LayerNorm
  SUMK_TRY(launch_layernorm(Y0, Y1, w->ln_w, w->ln_b, R, D, opts->eps, nullptr, stream));
  {  // 7: k1 + bias + ReLU
    GemmLaunch g;
    g.A = Y1; g.B[0] = w->W1; g.bias0[0] = w->b1; g.C = Z; g.probs = prow + 1; g.small_tile = st_d; g.total_tiles = gemm_tiles(R, D, st_d);
    g.xcd_M = R; g.xcd_N = D; g.lean = lean_rows; g.prof_tag = SUMK_PROF_GEMM_K1;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_BIAS_RELU, g, stream));
  }
  // 8: LayerNorm (same weights) + k2 + sigmoid
  SUMK_TRY(launch_ln_head(Z, w->ln_w, w->ln_b, w->w2, w->b2, scores, R, D, opts->eps, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
