// What the device-side evaluation kernels share (evaldev.hip: segment means + Spearman; evalkendall.hip: Kendall's tau-b): the limits of
// the per-video LDS tables and the pick-interval tables themselves.
#pragma once
#include "sumk_internal.h"
#include <math.h>

namespace sumk {

constexpr int ED_MAX_INT = 4096;     // pick intervals per video the block keeps in LDS (T <= 4095 steps)
constexpr int ED_MAX_USERS = 32;

// numpy's pairwise summation (numpy/core/src/umath/loops_utils.h.src), float32 -- same tree as csrc/evaltail.hip.  Shared by the segment
// means of evaldev.hip (upsampled scores) and annotate.hip (annotator rows): additions only, in one order.
__device__ inline float ed_pairwise_sum(const float* a, int n) {
  if (n < 8) {
    float r = 0.f;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  if (n <= 128) {
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return ed_pairwise_sum(a, n2) + ed_pairwise_sum(a + n2, n - n2);
}

// the interval tables of a video: interval i = frames [s_lo[i], s_hi[i]) takes score i (0 past the scores) -- eval.py:24-34.
// NT = threads of the block.
template <int NT = 256>
__device__ __forceinline__ void ed_intervals(const sumk_eval_dev_video& v, const float* __restrict__ scores, int n_int, int* s_lo, int* s_hi,
                                             float* s_val) {
  const int np_ = v.n_picks, n_frames = v.n_frames;
  for (int i = threadIdx.x; i < n_int; i += NT) {
    s_lo[i] = max(0, v.picks[i]);
    s_hi[i] = min(n_frames, i + 1 < np_ ? v.picks[i + 1] : n_frames);
    s_val[i] = i < v.n_steps ? scores[v.row0 + i] : 0.f;
  }
}

// ---- Kendall's tau-b, shared by the device kernel (evalkendall.hip) and the host threads (evaltail.hip): both sides end in the same
// integers and the same three float64 operations, so their results are equal bit for bit.
constexpr int KD_MAX_FRAMES = 16384;   // frames per video whose two key buffers the Kendall block keeps in LDS (2 x 64 KiB)
constexpr int KD_Y_BITS = 14;          // a dense annotator rank of such a video: < 2^14

// order-preserving integer image of a frame score: a < b <=> key(a) < key(b), -0.0 and +0.0 share one key (they are one tie group)
__host__ __device__ inline uint32_t kendall_float_key(float x) {
  if (x == 0.f) x = 0.f;
  union { float f; uint32_t u; } c;
  c.f = x;
  return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}

// tau-b from the pair counts, the operations and their order as scipy.stats.kendalltau has them (all counts below 2^53: exact as doubles)
__host__ __device__ inline double kendall_tau_b(int64_t cmd, int64_t tot, int64_t xtie, int64_t ytie) {
  if (xtie == tot || ytie == tot) return (double)NAN;          // a constant side (or fewer than two frames)
  const double tau = (double)cmd / sqrt((double)(tot - xtie)) / sqrt((double)(tot - ytie));
  return fmin(1.0, fmax(-1.0, tau));
}

}  // namespace sumk
