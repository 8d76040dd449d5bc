// Kendall's tau-b on the device-side evaluation tail: `evaluate_scores(metric="kendalltau")` of summarizer/utils/eval.py:49-72 with the
// scores still in HBM.  One workgroup per (video, annotator); every pair count is an integer, the three float64 operations of
// kendall_tau_b (evaldev_common.h) come last.
//
//   1. pick-interval tables as in evaldev.hip (ed_intervals) plus the group of frames no interval covers (value 0): <= 4097 groups
//   2. the groups' values, as order-preserving integers, are sorted; a group's x rank = the number of group values below its own
//      (equal floats -- a score of exactly 0.0 and the uncovered frames among them -- get one rank: one tie group)
//   3. key(frame) = x rank << 14 | dense annotator rank; the keys are merge-sorted in LDS
//   4. runs of equal keys give the joint ties, runs of equal x rank the ties of the machine scores
//   5. the y parts, now in (x, y) order, are merge-sorted again: the inversions are the discordant pairs
// A merge level places every element by one binary search in the sibling run (its rank there + its own position), which for an
// element of a left run is also its number of cross inversions: O(n log^2 n) LDS reads, no serial merge.  Two 64-KiB key buffers
// (ping-pong) hold up to KD_MAX_FRAMES frames; the group tables share the second buffer's space, which the first merge only writes
// after the keys are built.  131 KiB of LDS: dynamic, past the 64-KiB limit of static __shared__.
#include "evaldev_common.h"

#pragma clang fp contract(off)

namespace sumk {

constexpr int KD_TABLE = ED_MAX_INT + 8;                                  // entries of one group table (4097 used), a multiple of 4
constexpr size_t KD_BUF_BYTES = (size_t)KD_MAX_FRAMES * sizeof(uint32_t);
constexpr size_t KD_LDS_BYTES = KD_BUF_BYTES + (4 * (size_t)KD_TABLE * 4 > KD_BUF_BYTES ? 4 * (size_t)KD_TABLE * 4 : KD_BUF_BYTES);
static_assert(KD_LDS_BYTES <= 160 * 1024 - 1024, "the Kendall block must fit the CU's LDS");
static_assert(2 * (ED_MAX_INT + 1) <= KD_MAX_FRAMES, "the group sort ping-pongs inside the first key buffer");
static_assert(ED_MAX_INT + 1 < (1 << (32 - KD_Y_BITS)) && KD_MAX_FRAMES <= (1 << KD_Y_BITS), "key = x rank << KD_Y_BITS | y rank");

// grid (ED_MAX_USERS, n_videos); tau[video * ED_MAX_USERS + user]
__global__ __launch_bounds__(KD_THREADS) void eval_kendall_kernel(const float* __restrict__ scores, const sumk_eval_dev_video* __restrict__ vids,
                                                                   const sumk_eval_dev_kendall* __restrict__ kds, double* __restrict__ tau,
                                                                   int64_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kd_lds[];
  __shared__ long long s_red[KD_THREADS / 64][3];
  uint32_t* const buf_a = reinterpret_cast<uint32_t*>(kd_lds);
  uint32_t* const buf_b = reinterpret_cast<uint32_t*>(kd_lds + KD_BUF_BYTES);
  int* const s_lo = reinterpret_cast<int*>(buf_b);             // the group tables live where the first frame-key merge will write
  int* const s_hi = s_lo + KD_TABLE;
  float* const s_val = reinterpret_cast<float*>(s_hi + KD_TABLE);
  uint32_t* const s_xr = reinterpret_cast<uint32_t*>(s_val + KD_TABLE);
  const sumk_eval_dev_video v = vids[blockIdx.y];
  const sumk_eval_dev_kendall k = kds[blockIdx.y];
  const int tid = threadIdx.x, u = blockIdx.x, n = v.n_frames, np_ = v.n_picks;
  if (v.n_users > ED_MAX_USERS || u >= v.n_users) return;     // (more annotators than slots: the final kernel writes the video's NaN)
  const bool sentinel = np_ == 0 || v.picks[np_ - 1] != n;
  const int n_int = np_ - 1 + (sentinel ? 1 : 0);
  // fixed-size LDS: a descriptor past it (the host wrapper declines such videos) writes NaN and touches nothing else
  if (n_int > ED_MAX_INT || n_int < 0 || n > KD_MAX_FRAMES || n < 0 || k.y_dense == nullptr || k.ytie == nullptr) {
    if (tid == 0) {
      tau[(size_t)blockIdx.y * ED_MAX_USERS + u] = nan("");
      if (counts != nullptr) for (int q = 0; q < 4; ++q) counts[4 * (k.counts0 + u) + q] = -1;
    }
    return;
  }
  // ---- 1, 2: groups and their x ranks
  ed_intervals<KD_THREADS>(v, scores, n_int, s_lo, s_hi, s_val);
  if (tid == 0) { s_lo[n_int] = 0; s_hi[n_int] = 0; s_val[n_int] = 0.f; }      // the uncovered frames' group (its frames: whatever no interval holds)
  __syncthreads();
  const int n_grp = n_int + 1;
  for (int i = tid; i < n_grp; i += KD_THREADS) buf_a[i] = kendall_float_key(s_val[i]);
  __syncthreads();
  long long unused = 0;
  const uint32_t* sorted = kd_merge_sort(buf_a, buf_a + KD_MAX_FRAMES / 2, n_grp, unused);
  for (int i = tid; i < n_grp; i += KD_THREADS) s_xr[i] = (uint32_t)kd_lower(sorted, n_grp, kendall_float_key(s_val[i]));
  __syncthreads();
  // ---- 3: frame keys.  Picks ascend (checked by the host wrapper), so s_lo does: the interval of frame f is the last one that starts at
  // or before f (empty intervals of repeated picks are passed over); a frame outside it belongs to the uncovered group.
  const int32_t* y = k.y_dense + (size_t)u * n;
  for (int f = tid; f < n; f += KD_THREADS) {
    int g = kd_upper(reinterpret_cast<const uint32_t*>(s_lo), n_int, (uint32_t)f) - 1;      // (s_lo >= 0: the unsigned comparison is the signed one)
    if (g < 0 || f >= s_hi[g]) g = n_int;
    buf_a[f] = (s_xr[g] << KD_Y_BITS) | ((uint32_t)y[f] & ((1u << KD_Y_BITS) - 1u));
  }
  __syncthreads();
  uint32_t* key = kd_merge_sort(buf_a, buf_b, n, unused);
  uint32_t* other = key == buf_a ? buf_b : buf_a;
  // ---- 4: tied pairs, t (t - 1) / 2 per run, counted at the run's first element
  long long xtie = 0, ntie = 0, dis = 0;
  for (int i = tid; i < n; i += KD_THREADS) {
    const uint32_t c = key[i];
    if (i == 0 || key[i - 1] != c) {
      const long long t = kd_upper(key + i, n - i, c);
      ntie += t * (t - 1) / 2;
    }
    const uint32_t x0 = c >> KD_Y_BITS << KD_Y_BITS;
    if (i == 0 || key[i - 1] < x0) {
      const long long t = kd_lower(key + i, n - i, x0 + (1u << KD_Y_BITS));
      xtie += t * (t - 1) / 2;
    }
  }
  __syncthreads();
  // ---- 5: discordant pairs
  for (int i = tid; i < n; i += KD_THREADS) key[i] &= (1u << KD_Y_BITS) - 1u;
  __syncthreads();
  kd_merge_sort(key, other, n, dis);
  // integer sums: any order gives the same result
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    xtie += __shfl_xor(xtie, m, 64); ntie += __shfl_xor(ntie, m, 64); dis += __shfl_xor(dis, m, 64);
  }
  if (lane == 0) { s_red[wave][0] = xtie; s_red[wave][1] = ntie; s_red[wave][2] = dis; }
  __syncthreads();
  if (tid == 0) {
    xtie = ntie = dis = 0;
    for (int w = 0; w < KD_THREADS / 64; ++w) { xtie += s_red[w][0]; ntie += s_red[w][1]; dis += s_red[w][2]; }
    const int64_t tot = (int64_t)n * (n - 1) / 2, ytie = k.ytie[u];
    const int64_t cmd = tot - xtie - ytie + ntie - 2 * dis;
    tau[(size_t)blockIdx.y * ED_MAX_USERS + u] = kendall_tau_b(cmd, tot, xtie, ytie);
    if (counts != nullptr) {
      int64_t* c = counts + 4 * (k.counts0 + u);
      c[0] = cmd; c[1] = xtie; c[2] = ytie; c[3] = ntie;
    }
  }
}

// one thread per video: the mean over its annotators
__global__ __launch_bounds__(64) void eval_kendall_final_kernel(const sumk_eval_dev_video* __restrict__ vids, const double* __restrict__ tau,
                                                                double* __restrict__ corr, int n_videos) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_videos) return;
  const int nu = vids[i].n_users;
  corr[i] = nu > 0 && nu <= ED_MAX_USERS ? np_pairwise_leaf(tau + (size_t)i * ED_MAX_USERS, nu) / (double)nu : nan("");
}

}  // namespace sumk

extern "C" size_t sumk_eval_device_kendall_scratch_bytes(int32_t n_videos, int64_t total_frames) {
  // one tau per (video, annotator slot); the keys never leave LDS, so the frame count adds nothing (a negative one is an error: 0)
  if (n_videos <= 0 || total_frames < 0) return 0;
  return (size_t)n_videos * sumk::ED_MAX_USERS * sizeof(double);
}

extern "C" int sumk_eval_device_kendall(const float* scores_dev, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_kendall* kendall_dev,
                                        int32_t n_videos, void* scratch_dev, double* corr_dev, int64_t* counts_dev, void* stream) {
  using namespace sumk;
  SUMK_ARG(n_videos >= 0, "eval_device_kendall: n_videos=%d", n_videos);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(scores_dev && videos_dev && kendall_dev && scratch_dev && corr_dev, "eval_device_kendall: null pointer");
  SUMK_ARG(n_videos <= 65535, "eval_device_kendall: n_videos=%d (at most 65535 per call)", n_videos);
  SUMK_TRY(lds_opt_in<eval_kendall_kernel>((int)KD_LDS_BYTES));
  hipLaunchKernelGGL(eval_kendall_kernel, dim3(ED_MAX_USERS, n_videos), dim3(KD_THREADS), KD_LDS_BYTES, (hipStream_t)stream, scores_dev, videos_dev,
                     kendall_dev, (double*)scratch_dev, counts_dev);
  hipLaunchKernelGGL(eval_kendall_final_kernel, dim3((n_videos + 63) / 64), dim3(64), 0, (hipStream_t)stream, videos_dev, (const double*)scratch_dev,
                     corr_dev, n_videos);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
