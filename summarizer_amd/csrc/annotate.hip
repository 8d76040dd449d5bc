// Dataset records from raw annotations: the frame-level arithmetic in front of the key-shot selection (include/sumk.h, sumk_annotate).
// The reference reads gtscore / user_scores / user_summary / gtsummary that were prepared offline (summarizer/datasets/README.md:50-74);
// this unit is that preparation for a batch of videos whose annotations are in HBM, chained by summarizer_amd/utils/annotate.py into
// sumk_eval_device_segments (segment means of gtscore) and sumk_eval_device_select (one knapsack / rank problem per annotator row).
//
//   annotate_frames_kernel   one thread per frame, the annotators of that frame in order: user rows, consensus.  One pass over the
//                            U x n_frames floats, coalesced along the frames; the sum over annotators is sequential by definition.
//   annotate_video_kernel    one workgroup per video: min / max of the consensus at the picks (exact in any order), gtscore, then one
//                            thread per (annotator, segment) mean on the rows the first kernel wrote (np_pairwise_sum, the tree of
//                            evaldev.hip).  Stream order is the only dependency between the two: no atomics, no cooperative launch.
//   annotate_gtsummary_kernel  gtsummary[t] = frame summary of gtscore at picks[t].
// The specification is tests/annotate_ref.py, bit for bit: float32 operations in the stated order, compiled without FMA contraction.
#include "evaldev_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace sumk {

namespace {
constexpr int AN_THREADS = 256;
constexpr int AN_MAX_USERS = SUMK_SELECT_MAX_USERS;
constexpr int AN_MAX_PICKS = SUMK_ANNOTATE_MAX_PICKS;
constexpr int AN_MAX_SEGS = SUMK_SELECT_MAX_SEGS;
constexpr int AN_MAX_FRAMES = 1 << 24;       // the limit of sumk_eval_device_select; counts of annotators and frames stay exact in float32
constexpr int AN_MAX_VIDEOS = 65535;         // grid.y
static_assert(AN_MAX_USERS == ED_MAX_USERS && AN_MAX_PICKS + 1 == ED_MAX_INT, "limits of the kernels sumk_annotate chains into");

// what the entry point checks on the host copy, again on the device copy: a descriptor that disagrees is skipped
__device__ __forceinline__ bool an_within_limits(const sumk_annotate_video& v) {
  return v.anno != nullptr && v.picks != nullptr && v.cps != nullptr && v.n_users >= 1 && v.n_users <= AN_MAX_USERS && v.n_frames >= 1 &&
         v.n_frames <= AN_MAX_FRAMES && v.n_picks >= 1 && v.n_picks <= AN_MAX_PICKS && v.n_segs >= 1 && v.n_segs <= AN_MAX_SEGS;
}
__device__ __forceinline__ int an_pick(const sumk_annotate_video& v, int t) { return max(0, min(v.n_frames - 1, v.picks[t])); }
}  // namespace

// grid (ceil(longest video / AN_THREADS), n_videos)
__global__ __launch_bounds__(AN_THREADS) void annotate_frames_kernel(const sumk_annotate_video* __restrict__ vids, int protocol, float lo,
                                                                     float range, float* __restrict__ user, float* __restrict__ consensus) {
  const sumk_annotate_video v = vids[blockIdx.y];
  const int f = blockIdx.x * AN_THREADS + threadIdx.x;
  if (!an_within_limits(v) || f >= v.n_frames) return;
  const int U = v.n_users;
  const size_t nf = (size_t)v.n_frames;
  const float* a = v.anno + f;
  float* out = user + v.user0 + f;
  if (protocol == SUMK_ANNOTATE_SCORES) {
    float sum = 0.f;
    for (int u = 0; u < U; ++u) {
      const float x = a[u * nf];
      sum += x;
      out[u * nf] = (x - lo) / range;
    }
    consensus[v.frame0 + f] = sum / (float)U;
  } else {
    int cnt = 0;
    for (int u = 0; u < U; ++u) {
      const bool on = a[u * nf] > 0.f;
      cnt += on ? 1 : 0;
      out[u * nf] = on ? 1.f : 0.f;
    }
    consensus[v.frame0 + f] = (float)cnt / (float)U;
  }
}

// grid (n_videos)
__global__ __launch_bounds__(AN_THREADS) void annotate_video_kernel(const sumk_annotate_video* __restrict__ vids, int protocol,
                                                                    const float* __restrict__ user, const float* __restrict__ consensus,
                                                                    float* __restrict__ gtscore, float* __restrict__ seg_means) {
  __shared__ float s_mn[AN_THREADS / 64], s_mx[AN_THREADS / 64];
  const sumk_annotate_video v = vids[blockIdx.x];
  if (!an_within_limits(v)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, np_ = v.n_picks, n_frames = v.n_frames;
  const float* cons = consensus + v.frame0;
  float* gt = gtscore + v.pick0;
  if (protocol != SUMK_ANNOTATE_SCORES) {
    for (int t = tid; t < np_; t += AN_THREADS) gt[t] = cons[an_pick(v, t)];
    return;
  }
  // ---- min-max normalisation of the consensus at the picks (min and max of finite floats do not depend on the order)
  float mn = INFINITY, mx = -INFINITY;
  for (int t = tid; t < np_; t += AN_THREADS) { const float g = cons[an_pick(v, t)]; mn = fminf(mn, g); mx = fmaxf(mx, g); }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { mn = fminf(mn, __shfl_xor(mn, m, 64)); mx = fmaxf(mx, __shfl_xor(mx, m, 64)); }
  if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
  __syncthreads();
  mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
  mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
  const float span = mx - mn;
  for (int t = tid; t < np_; t += AN_THREADS) gt[t] = mx == mn ? 0.f : (cons[an_pick(v, t)] - mn) / span;
  // ---- float32 segment means of every annotator row (eval.py:91-94 on frame-level scores), one thread per (annotator, segment)
  const int n_segs = v.n_segs, n_means = v.n_users * n_segs;
  for (int i = tid; i < n_means; i += AN_THREADS) {
    const int u = i / n_segs, s = i - u * n_segs;
    const int lo = max(0, min(n_frames, v.cps[2 * s])), hi = max(lo, min(n_frames, v.cps[2 * s + 1] + 1));
    const float* row = user + v.user0 + (size_t)u * n_frames;
    seg_means[v.seg0 + i] = hi > lo ? np_pairwise_sum(row + lo, hi - lo) / (float)(hi - lo) : 0.f;
  }
}

// grid (ceil(AN_MAX_PICKS / AN_THREADS), n_videos)
__global__ __launch_bounds__(AN_THREADS) void annotate_gtsummary_kernel(const sumk_annotate_video* __restrict__ vids,
                                                                        const float* __restrict__ frame_summary, float* __restrict__ gtsummary) {
  const sumk_annotate_video v = vids[blockIdx.y];
  const int t = blockIdx.x * AN_THREADS + threadIdx.x;
  if (!an_within_limits(v) || t >= v.n_picks) return;
  gtsummary[v.pick0 + t] = frame_summary[v.gtsum0 + an_pick(v, t)];
}

namespace {
// the checks both entries share; *max_frames / *max_picks: the longest video of the call
int an_check(const char* what, const sumk_annotate_video* videos_host, int n_videos, int64_t pick_total, int* max_frames, int* max_picks) {
  SUMK_ARG(n_videos <= AN_MAX_VIDEOS, "%s: %d videos (at most %d per call)", what, n_videos, AN_MAX_VIDEOS);
  SUMK_ARG(pick_total >= 0, "%s: pick_total=%lld", what, (long long)pick_total);
  int mf = 0, mp = 0;
  for (int i = 0; i < n_videos; ++i) {
    const sumk_annotate_video& h = videos_host[i];
    SUMK_ARG(h.anno && h.picks && h.cps, "%s: video %d: null annotations / picks / change points", what, i);
    SUMK_ARG(h.n_users >= 1 && h.n_users <= AN_MAX_USERS, "%s: video %d has %d annotators (1 .. %d supported)", what, i, h.n_users, AN_MAX_USERS);
    SUMK_ARG(h.n_frames >= 1 && h.n_frames <= AN_MAX_FRAMES, "%s: video %d has %d frames (1 .. %d supported)", what, i, h.n_frames, AN_MAX_FRAMES);
    SUMK_ARG(h.n_picks >= 1 && h.n_picks <= AN_MAX_PICKS, "%s: video %d has %d picks (1 .. %d supported)", what, i, h.n_picks, AN_MAX_PICKS);
    SUMK_ARG(h.n_segs >= 1 && h.n_segs <= AN_MAX_SEGS, "%s: video %d has %d segments (1 .. %d supported)", what, i, h.n_segs, AN_MAX_SEGS);
    SUMK_ARG(h.reserved == 0, "%s: video %d: the reserved field must be 0", what, i);
    SUMK_ARG(h.summary_len == h.n_frames, "%s: video %d: the segments hold %d frames, the video %d (they must tile it)", what, i, h.summary_len,
             h.n_frames);
    SUMK_ARG(h.pick0 >= 0 && h.pick0 + h.n_picks <= pick_total, "%s: video %d: picks [%lld, +%d) outside the %lld entries given", what, i,
             (long long)h.pick0, h.n_picks, (long long)pick_total);
    mf = h.n_frames > mf ? h.n_frames : mf; mp = h.n_picks > mp ? h.n_picks : mp;
  }
  *max_frames = mf; *max_picks = mp;
  return SUMK_OK;
}
}  // namespace

}  // namespace sumk

using namespace sumk;

extern "C" int sumk_annotate(const sumk_annotate_video* videos_dev, const sumk_annotate_video* videos_host, int32_t n_videos, int32_t protocol,
                             float lo, float hi, float* user_dev, int64_t user_total, float* consensus_dev, int64_t frame_total,
                             float* gtscore_dev, int64_t pick_total, float* seg_means_dev, int64_t seg_total, void* stream) {
  SUMK_ARG(n_videos >= 0, "annotate: n_videos=%d", n_videos);
  SUMK_ARG(protocol == SUMK_ANNOTATE_SCORES || protocol == SUMK_ANNOTATE_SUMMARIES, "annotate: protocol %d (0 = scores, 1 = summaries)", protocol);
  const bool scores = protocol == SUMK_ANNOTATE_SCORES;
  // (written so that a NaN bound fails too)
  SUMK_ARG(!scores || (hi > lo && hi - lo < INFINITY && hi - lo > 0.f), "annotate: score range [%g, %g] must be finite with hi > lo", (double)lo, (double)hi);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(videos_dev && videos_host && user_dev && consensus_dev && gtscore_dev && (seg_means_dev || !scores), "annotate: null pointer");
  SUMK_ARG(user_total >= 0 && frame_total >= 0 && seg_total >= 0, "annotate: negative output size");
  int max_frames = 0, max_picks = 0;
  SUMK_TRY(an_check("annotate", videos_host, n_videos, pick_total, &max_frames, &max_picks));
  for (int i = 0; i < n_videos; ++i) {
    const sumk_annotate_video& h = videos_host[i];
    SUMK_ARG(h.user0 >= 0 && h.user0 + (int64_t)h.n_users * h.n_frames <= user_total, "annotate: video %d: rows [%lld, +%d x %d) outside the %lld entries given", i,
             (long long)h.user0, h.n_users, h.n_frames, (long long)user_total);
    SUMK_ARG(h.frame0 >= 0 && h.frame0 + h.n_frames <= frame_total, "annotate: video %d: frames [%lld, +%d) outside the %lld entries given", i,
             (long long)h.frame0, h.n_frames, (long long)frame_total);
    SUMK_ARG(!scores || (h.seg0 >= 0 && h.seg0 + (int64_t)h.n_users * h.n_segs <= seg_total),
             "annotate: video %d: segment means [%lld, +%d x %d) outside the %lld entries given", i, (long long)h.seg0, h.n_users, h.n_segs, (long long)seg_total);
  }
  // the frame pass launches ceil(longest video / 256) x n_videos blocks of 256 threads: a grid has to stay below 2^32 threads
  const int64_t frame_blocks = (int64_t)((max_frames + AN_THREADS - 1) / AN_THREADS) * n_videos;
  SUMK_ARG(frame_blocks * AN_THREADS < ((int64_t)1 << 32), "annotate: %d videos x %d frames (the longest) is past one launch (2^32 threads): split the batch",
           n_videos, max_frames);
  const float range = hi - lo;
  hipLaunchKernelGGL(annotate_frames_kernel, dim3((max_frames + AN_THREADS - 1) / AN_THREADS, n_videos), dim3(AN_THREADS), 0, (hipStream_t)stream,
                     videos_dev, protocol, lo, range, user_dev, consensus_dev);
  SUMK_HIP(hipGetLastError());
  hipLaunchKernelGGL(annotate_video_kernel, dim3(n_videos), dim3(AN_THREADS), 0, (hipStream_t)stream, videos_dev, protocol,
                     (const float*)user_dev, (const float*)consensus_dev, gtscore_dev, seg_means_dev);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_annotate_gtsummary(const sumk_annotate_video* videos_dev, const sumk_annotate_video* videos_host, int32_t n_videos,
                                       const float* frame_summary_dev, int64_t frame_summary_total, float* gtsummary_dev, int64_t pick_total,
                                       void* stream) {
  SUMK_ARG(n_videos >= 0, "annotate_gtsummary: n_videos=%d", n_videos);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(videos_dev && videos_host && frame_summary_dev && gtsummary_dev, "annotate_gtsummary: null pointer");
  SUMK_ARG(frame_summary_total >= 0, "annotate_gtsummary: frame_summary_total=%lld", (long long)frame_summary_total);
  int max_frames = 0, max_picks = 0;
  SUMK_TRY(an_check("annotate_gtsummary", videos_host, n_videos, pick_total, &max_frames, &max_picks));
  for (int i = 0; i < n_videos; ++i) {
    const sumk_annotate_video& h = videos_host[i];
    SUMK_ARG(h.gtsum0 >= 0 && h.gtsum0 + h.n_frames <= frame_summary_total, "annotate_gtsummary: video %d: frames [%lld, +%d) outside the %lld entries given", i,
             (long long)h.gtsum0, h.n_frames, (long long)frame_summary_total);
  }
  hipLaunchKernelGGL(annotate_gtsummary_kernel, dim3((max_picks + AN_THREADS - 1) / AN_THREADS, n_videos), dim3(AN_THREADS), 0, (hipStream_t)stream,
                     videos_dev, frame_summary_dev, gtsummary_dev);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
