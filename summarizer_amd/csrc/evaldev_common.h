// What the device-side evaluation kernels share (evaldev.hip: segment means + Spearman; evalkendall.hip: Kendall's tau-b; evalselect.hip:
// key shots + F-scores; evallong.hip: both for long videos; agreement.hip: inter-annotator agreement): the limits of the per-video LDS
// tables, numpy's pairwise sum, the pick-interval tables themselves, the LDS merge sort of the Kendall blocks, the steps of the key-shot
// selection and the F-score arithmetic.
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
// the tree: the leaf up to 128 values, above that the halves split at a multiple of 8.  N = the caller's own length type (int in the
// kernels, whose recursion then keeps 32-bit lengths on its call stack; int64_t on the host).
template <class T, class N>
__host__ __device__ inline T np_pairwise_tree(const T* a, N n) {
  if (n <= 128) return np_pairwise_leaf(a, (int)n);
  N n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_tree(a, n2) + np_pairwise_tree(a + n2, n - n2);
}
// any n, what `a.sum()` of a contiguous array gives: numpy hands its reduction loop at most one buffer of the array at a time --
// NP_BUFSIZE = 8192 elements, numpy.getbufsize()'s default, of either type -- so the tree spans one such block and the blocks' sums are
// added one after the other, in order.  Up to 8192 values this is the tree itself.
constexpr int NP_BUFSIZE = 8192;
template <class T, class N>
__host__ __device__ inline T np_pairwise_sum(const T* a, N n) {
  if (n <= (N)NP_BUFSIZE) return np_pairwise_tree(a, n);
  T r = np_pairwise_tree(a, (N)NP_BUFSIZE);
  for (N i = NP_BUFSIZE; i < n; i += NP_BUFSIZE) r += np_pairwise_tree(a + i, n - i < (N)NP_BUFSIZE ? n - i : (N)NP_BUFSIZE);
  return r;
}

// The tree of n <= NP_BUFSIZE values by a block of 1 << DEPTH threads (evallong.hip: a workgroup per segment).  The block walks the split
// rule above DEPTH levels down, thread t taking the turns its bits spell (the most significant first), each thread sums the subtree it
// arrives at with np_pairwise_tree, and the partial sums are joined in LDS, deepest level first, left + right: the additions of the
// one-thread tree, each once, on the same operands in the same order -- the same bits.  A node of 128 values or fewer above the cut is a
// leaf of the tree: the thread on its leftmost path sums it, the others below it hold nothing.  Every thread of the block calls it
// (barriers inside; a, n block-uniform); s_sum / s_has: 1 << DEPTH LDS entries each.  The result is thread 0's.
template <int DEPTH>
__device__ inline float np_pairwise_tree_block(const float* a, int n, float* s_sum, uint8_t* s_has) {
  constexpr int NT = 1 << DEPTH;
  const int tid = threadIdx.x;
  int off = 0, len = n;
  bool has = true;
  for (int level = 0; level < DEPTH; ++level) {
    if (len <= 128) { has = (tid & ((1 << (DEPTH - level)) - 1)) == 0; break; }
    int n2 = len / 2;
    n2 -= n2 % 8;
    if ((tid >> (DEPTH - 1 - level)) & 1) { off += n2; len -= n2; } else len = n2;
  }
  s_sum[tid] = has ? np_pairwise_tree(a + off, len) : 0.f;
  s_has[tid] = has ? 1 : 0;
  __syncthreads();
  // at stride st the node on whose leftmost path thread t lies takes its right child, if the tree split there
  for (int st = 1; st < NT; st <<= 1) {
    if ((tid & (2 * st - 1)) == 0 && s_has[tid + st]) s_sum[tid] = s_sum[tid] + s_sum[tid + st];
    __syncthreads();
  }
  return s_sum[0];
}
// np_pairwise_sum of n > NP_BUFSIZE values by a block of NT threads: a buffer block per thread (thread t takes blocks t, t + NT, ...), the
// blocks' sums in LDS, then thread 0 adds them in order.  s_part: ceil(n / NP_BUFSIZE) LDS entries.  Every thread of the block calls it
// (one barrier inside); the result is thread 0's.
template <int NT>
__device__ inline float np_pairwise_sum_blocks(const float* a, int n, float* s_part) {
  const int n_blocks = (n + NP_BUFSIZE - 1) / NP_BUFSIZE;
  for (int b = threadIdx.x; b < n_blocks; b += NT) s_part[b] = np_pairwise_tree(a + b * NP_BUFSIZE, min(NP_BUFSIZE, n - b * NP_BUFSIZE));
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) {
    r = s_part[0];
    for (int b = 1; b < n_blocks; ++b) r += s_part[b];
  }
  return r;
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

// ---- what the two key-shot selections share (evalselect.hip: one workgroup per video; evallong.hip: the chip-wide form)
constexpr int SEL_THREADS = 1024;                            // one segment per thread in the scans
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_MAX_SEGS = SUMK_SELECT_MAX_SEGS;
constexpr int SEL_MAX_USERS = SUMK_SELECT_MAX_USERS;
constexpr int SEL_MAX_FRAMES = 1 << 24;                      // counts of frames stay exact in float32
static_assert(SEL_MAX_SEGS == SEL_THREADS && SEL_MAX_USERS == ED_MAX_USERS, "limits of the select kernels");

// exclusive prefix sum over the block of one value per thread, *total = the block's sum; s_wsum: SEL_WAVES entries
__device__ __forceinline__ long long sel_scan(long long x, long long* s_wsum, long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(incl, o);
    if (lane >= o) incl += u;
  }
  __syncthreads();                           // (the previous scan's readers are done with s_wsum)
  if (lane == 63) s_wsum[wave] = incl;
  __syncthreads();
  long long base = 0, tot = 0;
  for (int q = 0; q < SEL_WAVES; ++q) { const long long c = s_wsum[q]; base += q < wave ? c : 0; tot += c; }
  *total = tot;
  return base + incl - x;
}

// The integers of a video's selection, one thread per segment (a block of SEL_THREADS; every thread calls it: barriers inside).
//   by segment:  w_all[s] = nfps[s] (0 for a negative one), start[s] = the prefix sum of the weights, clamped to len; start[n] = len
//   by position in the knapsack's pass (method 0; items with val > 0 and w <= cap, in segment order): live[pos] = the segment,
//                sv[pos] = its value (int64_t)((double)mean * 1000.0), swl[pos] = its weight
// The tables may be LDS or global memory; s_flag (2 ints) and s_wsum (SEL_WAVES) are LDS.  *m = items in the pass (0 when their values
// sum to 2^31 or more), *x = this thread's segment mean as a double.  Returns the video's status: 0, or 1 (a segment mean is not
// finite or past 1e12), 3 (a negative nfps, or nfps that do not sum to len), 2 (values past the int32 profit rows), in this precedence.
template <class LiveT>
__device__ __forceinline__ int sel_prepare(const sumk_eval_dev_select& v, int n, int cap, int len, int* s_flag, long long* s_wsum, int* w_all,
                                           int* start_tab, LiveT* live_tab, int* sv, int* swl, int* m_out, double* x_out) {
  const int tid = threadIdx.x;
  if (tid < 2) s_flag[tid] = 0;
  __syncthreads();
  // ---- values and weights (eval_one: int64 truncation of the double product)
  long long val = 0; int w = 0; double x = 0.0;
  if (tid < n) {
    const float mean = v.seg_means[tid];
    w = v.nfps[tid];
    x = (double)mean;
    if (!(fabs(x) <= 1e12)) { s_flag[0] = 1; x = 0.0; }          // NaN, infinite, or past what the cast to int64 defines
    if (w < 0) { s_flag[1] = 1; w = 0; }
    val = (long long)(x * 1000.0);
    w_all[tid] = w;
  }
  long long total;
  const long long start = sel_scan((long long)w, s_wsum, &total);
  if (tid < n) start_tab[tid] = (int)(start < (long long)len ? start : (long long)len);
  if (tid == 0) { start_tab[n] = len; if (total != (long long)len) s_flag[1] = 1; }
  int m = 0;
  if (v.method == 0) {
    const bool live = tid < n && val > 0 && w <= cap;
    long long possum, cnt;
    sel_scan(live ? val : 0, s_wsum, &possum);
    const long long pos = sel_scan(live ? 1 : 0, s_wsum, &cnt);
    if (possum >= ((long long)1 << 31) && tid == 0) s_flag[0] = s_flag[0] ? 1 : 2;
    m = possum < ((long long)1 << 31) ? (int)cnt : 0;
    if (live && m > 0) { live_tab[pos] = (LiveT)tid; sv[pos] = (int)val; swl[pos] = w; }
  }
  __syncthreads();
  *m_out = m; *x_out = x;
  return s_flag[0] == 1 ? 1 : s_flag[1] ? 3 : s_flag[0];          // 1: segment mean; 3: nfps; 2: values past int32 rows
}

// the segment that owns summary entry f: the last s with start[s] <= f (empty segments share their start with the next one)
__device__ __forceinline__ int sel_segment_of(const int* s_start, int n, int f) {
  int lo = 0, hi = n;                        // start[lo] <= f < start[hi] (start[n] = summary_len > f)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s_start[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// Backtrack of the one-pass knapsack on one wave (every lane of it calls this): bit (j, c) of `bits` = the item at position j improved
// capacity c, `words` 64-bit words per item.  From (k = n, rem = cap): s = the segment of the largest position < kpos whose bit is set
// at rem, segment 0 if there is none; rem -= its weight; s is selected if rem >= 0; repeat while rem > 0 and k > 0.  The scan for the
// largest set bit only ever moves down.  kpos = items in the pass (0 when no pass ran); w0 = the weight of segment 0.
template <class LiveT>
__device__ __forceinline__ void sel_backtrack(const unsigned long long* bits, int words, int n, int cap, int kpos, const LiveT* live_tab, const int* swl,
                                              int w0, uint8_t* sel) {
  const int lane = threadIdx.x & 63;
  int rem = cap, k = n;
  while (rem > 0 && k > 0) {
    int found = -1;
    for (int hi = kpos; hi > 0 && found < 0; hi -= 64) {
      const int j = hi - 1 - lane;
      const bool b = j >= 0 && ((bits[(size_t)j * words + (rem >> 6)] >> (rem & 63)) & 1ull) != 0;
      const unsigned long long mask = __ballot(b);
      if (mask) found = hi - __ffsll((long long)mask);
    }
    const int s = found >= 0 ? (int)live_tab[found] : 0;
    rem -= found >= 0 ? swl[found] : w0;
    k = s; kpos = found > 0 ? found : 0;
    if (rem >= 0 && lane == 0) sel[s] = 1;
  }
}

// eval_one's rank walk: stable_sort by ascending double score walked from the back = descending score, the larger index first among
// equals; the sorted position by counting, the greedy walk (strict total + nfps < capacity) on one thread.  s_x (SEL_MAX_SEGS doubles)
// and s_order (SEL_MAX_SEGS ints) are LDS; x = this thread's score; every thread of the block calls it (barriers inside).
__device__ __forceinline__ void sel_rank_walk(double x, int n, int cap, const int* w_all, double* s_x, int* s_order, uint8_t* sel) {
  const int tid = threadIdx.x;
  if (tid < n) s_x[tid] = x;
  __syncthreads();
  if (tid < n) {
    int pos = 0;
    for (int j = 0; j < n; ++j) { const double y = s_x[j]; pos += (y < x || (y == x && j < tid)) ? 1 : 0; }
    s_order[pos] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    long long used = 0;
    for (int q = n - 1; q >= 0; --q) {
      const int i = s_order[q];
      if (used + w_all[i] < (long long)cap) { sel[i] = 1; used += w_all[i]; }
    }
  }
}

// ---- the F-score arithmetic evalselect.hip, evallong.hip and agreement.hip share
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
