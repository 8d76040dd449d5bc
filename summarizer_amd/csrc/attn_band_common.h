// Geometry of local attention on the band, shared by the scoring launches (attn_band.hip) and the training launches (attn_band_bwd.hip):
// strips of 64 query rows, one 64 x (k_hi - k_lo) rectangle per strip, 64-bit offsets.  See the head of attn_band.hip.
#pragma once
#include "sumk_internal.h"
#include <math.h>

namespace sumk {

// A video has at most 2^20 steps.  The limit is also EXACTLY what the dropout index of the attention weights can hold: the mask of
// entry (packed row, key) is drawn at index (packed_row << 20) | key_in_video, the dense kernel's index (vasnet_softmax_kernel), so
// the key takes the low 20 bits.  Raising AB_MAX_T would make two entries of one row share a mask.
constexpr int AB_MAX_T = 1048576;

// ---- sizes of one video; host and device must agree byte for byte, so both call these
struct ABandSizes { int64_t e, tiles_s; int32_t strips, pitch; };     // floats of logits, 64x64 logits tiles, strips, rectangle pitch

__host__ __device__ inline int ab_k_lo(int w, int r) { const int64_t v = (int64_t)64 * r - w; return v > 0 ? (int)v : 0; }
__host__ __device__ inline int ab_k_hi(int T, int w, int r) { const int64_t v = (int64_t)64 * r + 64 + w; return v < T ? (int)v : T; }
__host__ __device__ inline int ab_strip_tiles(int T, int w, int r) { return (ab_k_hi(T, w, r) - ab_k_lo(w, r) + 63) / 64; }
// logits tiles of strips 0 .. r - 1.  Strips that touch neither end of the video have 2 w + 64 keys each; only the (at most ~ w / 32 + 3)
// strips at the two ends are walked.
__host__ __device__ inline int64_t ab_tiles_before(int T, int w, int r) {
  const int64_t strips = ((int64_t)T + 63) / 64;
  int64_t i0 = ((int64_t)w + 63) / 64;                                  // first strip with 64 r - w >= 0
  int64_t i1 = (int64_t)T - 64 - w >= 0 ? ((int64_t)T - 64 - w) / 64 + 1 : 0;      // one past the last strip with 64 r + 64 + w <= T
  i0 = i0 < strips ? i0 : strips; i1 = i1 < strips ? i1 : strips; i1 = i1 > i0 ? i1 : i0;
  int64_t s = 0;
  const int64_t a = r < i0 ? r : i0;
  for (int64_t q = 0; q < a; ++q) s += ab_strip_tiles(T, w, (int)q);
  if (r > i0) s += ((r < i1 ? r : i1) - i0) * (((int64_t)2 * w + 64 + 63) / 64);
  for (int64_t q = i1; q < r; ++q) s += ab_strip_tiles(T, w, (int)q);
  return s;
}
__host__ __device__ inline ABandSizes aband_sizes(int T, int w) {
  ABandSizes z;
  const int64_t full = (int64_t)2 * w + 64;
  z.pitch = (int)(((T < full ? T : full) + 3) & ~(int64_t)3);
  z.strips = (T + 63) / 64;
  z.e = (int64_t)z.strips * 64 * z.pitch;
  z.tiles_s = ab_tiles_before(T, w, z.strips);
  return z;
}

struct ABSeq { int64_t e_off, tile_s0; int32_t row0, T, strip0, pitch; };               // one video
struct ABStrip { int64_t e_off; int32_t row0, rows, i0, k_lo, n_keys, pitch; };         // one strip: row0 = its first PACKED row, i0 = that row inside the video

// workspace of the band itself.  n_e rectangle buffers of `e_elems` floats (stride e_stride bytes) start at `e`: one when scoring, three
// (alpha, dropout(alpha) / dAlpha / dLogits, transposed rectangles) when training; n_tab problem tables of one entry per strip start at `prob`.
struct ABandWs {
  size_t e, e_stride, seq, strip, prob, prob_stride, total;
  int64_t e_elems, strips, tiles_s, tiles_c; int32_t w, keys_max, rows;
};

// `w` of the geometry: an aperture past the longest possible video sees every key, as AB_MAX_T does (and stays clear of int32 overflow)
inline int ab_clamp_w(int aperture) { return aperture < AB_MAX_T ? aperture : AB_MAX_T; }

// checks the batch and lays the band out behind `base` bytes (attn_band.hip)
int ab_carve(const char* who, int D, int n_seq, const int32_t* off, int aperture, size_t base, int n_e, int n_tab, ABandWs* L);
int ab_t_max(int n_seq, const int32_t* off);
int ab_check_operands(const char* who, int D, const void* const ptrs[], const int32_t lds[], int n);

// per video its offsets (attn_band.hip); the caller launches it before any strip table is built
__global__ void attn_band_seq_kernel(const int32_t* off, int n_seq, int w, ABSeq* seq);
// per strip its record and up to six GEMM problems.  A table is one of two shapes over the strip's rectangle at e_off:
//   "rect out"  C(rows, n_keys) = A[row0 ..] B[k_lo ..]^T  (NT, K = D): the logits (Q, K) and dAlphaD (dCTX, V)
//   "rect in"   C(rows, D) = rect(rows, n_keys) B[k_lo .. k_lo + n_keys)  (NN, K = n_keys EXACTLY): the context (alpha, V), dQ (dLogits, K) and,
//               on the TRANSPOSED rectangles, dV (alphaD^T, dCTX) and dK (dLogits^T, Q) -- the band is symmetric, so key strip c is seen by
//               exactly the query rows ab_k_lo(w, c) .. ab_k_hi(T, w, c): same count, same pitch, same e_off.
struct ABTab { GemmProb* prob; int32_t rect_out, lda, ldb, ldc; };      // rect_out: lda = A rows, ldb = B rows; rect in: ldb = B rows, ldc = C rows
struct ABSetup { const ABSeq* seq; ABStrip* strip; ABTab tab[6]; int32_t n_tab, w, D; };
__global__ void attn_band_strip_kernel(ABSetup a);
int ab_launch_setup(const ABandWs& L, char* ws, const int32_t* off_dev, int n_seq, int t_max, int D, const ABTab* tabs, int n_tab, hipStream_t stream);

__device__ __forceinline__ float ab_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float ab_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// One call of the attention on the band.  Scoring: alpha_test may be set, E2 / drop unused.  Training forward: E2 receives dropout(alpha)
// when drop.thr != 0 and the context is taken from it.
struct ABandCall {
  const float* Q; const float* K; const float* V; float* ctx; float* alpha;
  int32_t ldq, ldk, ldv, ldc, D, n_seq; const int32_t* off_dev; float scale; int32_t ignore_self, aperture;
};
// setup + logits + softmax + context of the scoring path; every argument has been checked (attn_band.hip)
int attn_band_launch(const ABandCall& c, const ABandWs& L, char* ws, int t_max, hipStream_t stream);
// the same, keeping alpha in rectangle buffer 0 and dropout(alpha) in buffer 1 (attn_band_bwd.hip)
int attn_band_train_launch(const ABandCall& c, const ABandWs& L, char* ws, int t_max, Drop drop, hipStream_t stream);
struct ABandBwdCall {
  const float* Q; const float* K; const float* V; const float* dctx; float* dQ; float* dK; float* dV;
  int32_t ldq, ldk, ldv, lddc, lddq, lddk, lddv, D, n_seq; const int32_t* off_dev; float scale; int32_t ignore_self;
};
int attn_band_bwd_launch(const ABandBwdCall& c, const ABandWs& L, char* ws, int t_max, Drop drop, hipStream_t stream);

}  // namespace sumk
