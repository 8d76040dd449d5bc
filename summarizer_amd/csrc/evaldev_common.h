// What the device-side evaluation kernels share (evaldev.hip: segment means + Spearman; evalkendall.hip: Kendall's tau-b; evalselect.hip:
// key shots + F-scores; agreement.hip: inter-annotator agreement): the limits of the per-video LDS tables, the pick-interval tables
// themselves, the LDS merge sort of the Kendall blocks and the F-score arithmetic.
#pragma once
#include "sumk_internal.h"
#include <math.h>

namespace sumk {

constexpr int ED_MAX_INT = 4096;     // pick intervals per video the block keeps in LDS (T <= 4095 steps)
constexpr int ED_MAX_USERS = 32;

// numpy's pairwise summation (numpy/core/src/umath/loops_utils.h.src), the one copy every bit-exact mean of the library goes through, host
// (evaltail.hip) and device, T = float or double.  Additions only, in one order: there is nothing for FMA contraction to fuse, so the
// contraction setting of the including unit (-ffp-contract=off, #pragma clang fp contract(off)) cannot change a result.
// np_pairwise_leaf: the unrolled block of n <= 128 values (below 8 a running sum; numpy starts that one from -0.0, which differs from +0
// only for an all -0.0 input).  Callers that know n <= 128 (the annotators of a video: at most ED_MAX_USERS) take it directly and stay
// free of device recursion.
template <class T>
__host__ __device__ inline T np_pairwise_leaf(const T* a, int n) {
  if (n < 8) {
    T r = (T)0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  T r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  }
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}
// any n: the leaf up to 128, above that the halves split at a multiple of 8.  N = the caller's own length type (int in the kernels, whose
// recursion then keeps 32-bit lengths on its call stack; int64_t on the host).
template <class T, class N>
__host__ __device__ inline T np_pairwise_sum(const T* a, N n) {
  if (n <= 128) return np_pairwise_leaf(a, (int)n);
  N n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
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

// ---- what the Kendall blocks of evalkendall.hip and agreement.hip share: the block size, the binary searches and the LDS merge sort
constexpr int KD_THREADS = 1024;

// elements of the sorted run a[0..n) below v / not above v
__device__ __forceinline__ int kd_lower(const uint32_t* a, int n, uint32_t v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; }
  return lo;
}
__device__ __forceinline__ int kd_upper(const uint32_t* a, int n, uint32_t v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (a[m] <= v) lo = m + 1; else hi = m; }
  return lo;
}

// Stable bottom-up merge sort of a[0..n) with b as the other buffer; returns the buffer that holds the result.  Every thread must call
// it (barriers inside); a, b and n are block-uniform.  inv collects this thread's share of the inversions of the input.
__device__ inline uint32_t* kd_merge_sort(uint32_t* a, uint32_t* b, int n, long long& inv) {
  for (int w = 1; w < n; w <<= 1) {
    for (int i = threadIdx.x; i < n; i += KD_THREADS) {
      const int s = i & ~(2 * w - 1), mid = min(s + w, n), end = min(s + 2 * w, n);
      const uint32_t v = a[i];
      int dst;
      if (i < mid) {
        const int c = kd_lower(a + mid, end - mid, v);      // right-run elements below v: they overtake it
        inv += c;
        dst = i + c;
      } else {
        dst = s + (i - mid) + kd_upper(a + s, mid - s, v);   // left-run elements not above v stay in front
      }
      b[dst] = v;
    }
    __syncthreads();
    uint32_t* t = a; a = b; b = t;
  }
  return a;
}

// ---- the F-score arithmetic evalselect.hip and agreement.hip share
// fscores<T> of csrc/evaltail.hip from the counts: msum = ones of the machine summary over the video's frames, ov[k] / gs[k] = the
// overlap with annotator k and the annotator's own count
template <typename T>
__device__ void sel_fscores(int msum, const int* ov, const int* gs, int n_users, T eps, T* f, double* f_avg, double* f_max) {
  const T m_sum = (T)msum;
  T best = (T)0;
  for (int k = 0; k < n_users; ++k) {
    const T overlap = (T)ov[k];
    const T precision = overlap / (T)(m_sum + eps);
    const float gsum = (float)gs[k];
    const T recall = overlap / (T)(float)(gsum + 1e-8f);
    f[k] = (precision == (T)0 && recall == (T)0) ? (T)0 : (((T)2 * precision) * recall) / (precision + recall);
    best = (k == 0 || best < f[k]) ? f[k] : best;
  }
  *f_avg = (double)(T)(np_pairwise_leaf(f, n_users) / (T)n_users);      // n_users <= ED_MAX_USERS
  *f_max = (double)best;
}

}  // namespace sumk
