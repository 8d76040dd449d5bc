// The device evaluation tail for long videos: upsample + segment means (sumk_eval_device_segments_long) and key-shot selection, summary
// expansion and F-scores (sumk_eval_device_select_long) without the per-video LDS tables of evaldev.hip / evalselect.hip, whose one
// workgroup per video stops at 4096 picks and a frame budget of 8191.  The specification is unchanged -- the host tail, bit for bit:
// eval_one / fscores of csrc/evaltail.hip and sumk_knapsack_dp of csrc/knapsack.hip -- and so are the descriptors, outputs and status codes.
//
//   upsample   frame-centric on a grid over (frame chunks, videos): frame f takes the score of the last pick interval i with picks[i] <= f
//              (binary search in the video's picks, which stay in HBM / L2).  For ascending picks this is the array the in-order interval
//              loop of eval_segments_kernel writes: interval i covers [picks[i], picks[i + 1]), an interval between equal picks is empty.
//   means      a workgroup per (video, segment), np_pairwise_sum of evaldev_common.h spread over it.  Up to NP_BUFSIZE = 8192 frames the sum
//              is one pairwise tree: np_pairwise_tree_block cuts it ML_DEPTH levels down, a subtree per thread, the partial sums joined
//              in tree order.  Past that numpy adds the trees of 8192-frame blocks one after the other: np_pairwise_sum_blocks, a block
//              per thread, the blocks' sums added in order by one thread.  Either way the additions of the one-thread np_pairwise_sum
//              that eval_segments_kernel runs, each once, in its order; then one division.
//   knapsack   the one-pass DP of evalselect.hip (sel_dp) as one launch per item position over (capacity chunks, videos): the launch of
//              item j reads profit row (j - 1) & 1 of the workspace (written by the launch before it; item 0 reads none: the row of no
//              items is all zero) and writes row j & 1 plus the improvement bits of (j, c).  Nothing waits inside a launch.
//   F-scores   the counts are integers: int32 per thread, per (video, frame chunk) partial counts in the workspace, added by a last
//              launch in chunk order (any order gives the same integers); then sel_fscores<float | double> as in evalselect.hip.
// This unit is compiled without FMA contraction, like evaldev.hip and evalselect.hip.
#include "evaldev_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace sumk {

namespace {
constexpr int EL_MAX_PICKS = SUMK_SEGMENTS_LONG_MAX_PICKS;
constexpr int EL_MAX_FRAMES = SUMK_SEGMENTS_LONG_MAX_FRAMES;
constexpr int UP_THREADS = 256, UP_PER_THREAD = 8, UP_CHUNK = UP_THREADS * UP_PER_THREAD;      // frames per upsample block
constexpr int ML_DEPTH = 8, ML_THREADS = 1 << ML_DEPTH;                                         // the cut of the pairwise tree

constexpr int SL_MAX_CAP = SUMK_SELECT_LONG_MAX_CAPACITY;
constexpr int SL_CHUNK = SUMK_SELECT_LONG_CHUNK;             // capacities per DP block
constexpr int SL_DP_THREADS = 256;
constexpr int SL_FCHUNKS = SUMK_SELECT_LONG_FRAME_CHUNKS;    // frame chunks per video at most (slots of partial counts)
constexpr int SL_FR_THREADS = 256;
constexpr int SL_FR_PER_BLOCK = 4096;                        // frames a chunk holds before the call takes more chunks
constexpr int SL_SLOTS = 2 * SEL_MAX_USERS + 1;              // per annotator {own count, overlap}, then the machine summary's count
static_assert(SL_CHUNK % (SL_DP_THREADS) == 0 && SL_MAX_CAP == SEL_MAX_FRAMES, "limits of the long select kernels");

// header of a video's item tables in the workspace, written by the prologue: what the later launches go by
enum { H_M = 0, H_STATUS, H_CAP, H_N, H_LEN, H_FRAMES, H_USERS, H_METHOD, H_INTS };

inline size_t sl_words(int64_t capacity) { return (size_t)((capacity + 1 + 63) / 64); }
inline size_t sl_bits_bytes(int max_segs, int max_cap) { return align_up((size_t)max_segs * sl_words(max_cap) * 8, 256); }
inline size_t sl_rows_bytes(int max_cap) { return align_up(2 * ((size_t)max_cap + 1) * 4, 256); }
inline size_t sl_items_bytes(int max_segs) { return align_up(((size_t)5 * max_segs + 1 + H_INTS) * 4, 256); }
inline size_t sl_counts_bytes() { return align_up((size_t)SL_FCHUNKS * SL_SLOTS * 4, 256); }
inline size_t sl_pitch(int max_segs, int max_cap) {
  return sl_bits_bytes(max_segs, max_cap) + sl_rows_bytes(max_cap) + sl_items_bytes(max_segs) + sl_counts_bytes();
}
}  // namespace

// ------------------------------------------------------------------------------------------------ segments
// grid (frame chunks, videos)
__global__ __launch_bounds__(UP_THREADS) void eval_upsample_long_kernel(const float* __restrict__ scores, const sumk_eval_dev_video* __restrict__ vids,
                                                                        float* __restrict__ frame_scratch) {
  const sumk_eval_dev_video v = vids[blockIdx.y];
  const int n_frames = v.n_frames, np_ = v.n_picks;
  // (the entry point checked the host copy; a device copy past the limits writes no frame: its segment means are NaN)
  if (np_ < 1 || np_ > EL_MAX_PICKS || n_frames < 1 || n_frames > EL_MAX_FRAMES) return;
  const int base = blockIdx.x * UP_CHUNK;
  if (base >= n_frames) return;
  const int32_t* __restrict__ picks = v.picks;
  const bool sentinel = picks[np_ - 1] != n_frames;
  const int n_int = np_ - 1 + (sentinel ? 1 : 0);
  float* fs = frame_scratch + v.frame0;
#pragma unroll
  for (int k = 0; k < UP_PER_THREAD; ++k) {
    const int f = base + k * UP_THREADS + threadIdx.x;
    if (f >= n_frames) break;
    int lo = 0, hi = n_int;                  // intervals [0, lo) start at or in front of f, intervals [hi, n_int) behind it
    while (lo < hi) { const int m = (lo + hi) >> 1; if (picks[m] <= f) lo = m + 1; else hi = m; }
    const int i = lo - 1;                    // -1: f lies in front of the first pick
    fs[f] = (i >= 0 && i < v.n_steps) ? scores[v.row0 + i] : 0.f;
  }
}

// grid (segments, videos)
__global__ __launch_bounds__(ML_THREADS) void eval_means_long_kernel(const sumk_eval_dev_video* __restrict__ vids, const float* __restrict__ frame_scratch,
                                                                     float* __restrict__ seg_means) {
  __shared__ float s_sum[ML_THREADS];
  __shared__ uint8_t s_has[ML_THREADS];
  __shared__ float s_part[EL_MAX_FRAMES / NP_BUFSIZE];      // a sum per buffer block of a segment past NP_BUFSIZE frames
  const sumk_eval_dev_video v = vids[blockIdx.y];
  const int s = blockIdx.x, tid = threadIdx.x, n_frames = v.n_frames;
  if (s >= v.n_segs) return;
  if (v.n_picks < 1 || v.n_picks > EL_MAX_PICKS || n_frames < 1 || n_frames > EL_MAX_FRAMES) {
    if (tid == 0) seg_means[v.seg0 + s] = nanf("");
    return;
  }
  const int lo = max(0, min(n_frames, v.cps[2 * s])), hi = max(lo, min(n_frames, v.cps[2 * s + 1] + 1)), n = hi - lo;
  if (n == 0) { if (tid == 0) seg_means[v.seg0 + s] = 0.f; return; }
  const float* a = frame_scratch + v.frame0 + lo;
  const float sum = n <= NP_BUFSIZE ? np_pairwise_tree_block<ML_DEPTH>(a, n, s_sum, s_has) : np_pairwise_sum_blocks<ML_THREADS>(a, n, s_part);
  if (tid == 0) seg_means[v.seg0 + s] = sum / (float)n;
}

// ------------------------------------------------------------------------------------------------ select
struct SelLongArgs {
  const sumk_eval_dev_select* vids;
  float* summary; uint8_t* selected; double* f_avg; double* f_max; int32_t* status;
  char* ws; size_t pitch, rows_off, items_off, counts_off;      // per video: improvement bits, two profit rows, item tables, partial counts
  long long summary_total, selected_total;
  int S, max_cap, max_frames;                                   // the call's largest n_segs / capacity / n_frames (host copy)
};

struct SelLongTables { int* hdr; int* sv; int* swl; int* live; int* w_all; int* start; };
__device__ __forceinline__ SelLongTables sl_tables(const SelLongArgs& a, int vi) {
  SelLongTables t;
  t.hdr = (int*)(a.ws + (size_t)vi * a.pitch + a.items_off);
  t.sv = t.hdr + H_INTS; t.swl = t.sv + a.S; t.live = t.swl + a.S; t.w_all = t.live + a.S; t.start = t.w_all + a.S;      // start: S + 1 entries
  return t;
}

// grid (videos)
__global__ __launch_bounds__(SEL_THREADS) void sel_long_prologue_kernel(SelLongArgs a) {
  __shared__ long long s_wsum[SEL_WAVES];
  __shared__ int s_flag[2];
  const int vi = blockIdx.x, tid = threadIdx.x;
  const sumk_eval_dev_select v = a.vids[vi];
  const SelLongTables t = sl_tables(a, vi);
  const int n = v.n_segs, cap = v.capacity, len = v.summary_len, n_frames = v.n_frames;
  const int n_users = (v.user_mask != nullptr && v.n_users > 0) ? v.n_users : 0;
  // the entry point checked the host copy of the descriptors; a device copy that disagrees with it must still write nothing out of bounds:
  // the workspace and the grids were sized by the host copy's largest values
  if (n < 1 || n > a.S || cap < 0 || cap > a.max_cap || n_users > SEL_MAX_USERS || len < 0 || n_frames < 1 || n_frames > a.max_frames ||
      (v.method != 0 && v.method != 1) || v.seg_means == nullptr || v.nfps == nullptr || v.summary0 < 0 ||
      v.summary0 + (long long)len > a.summary_total || v.sel0 < 0 || v.sel0 + (long long)n > a.selected_total) {
    if (tid == 0) { t.hdr[H_STATUS] = 4; t.hdr[H_M] = 0; a.status[vi] = 4; a.f_avg[vi] = nan(""); a.f_max[vi] = nan(""); }
    return;
  }
  int m; double x;
  const int bad = sel_prepare(v, n, cap, len, s_flag, s_wsum, t.w_all, t.start, t.live, t.sv, t.swl, &m, &x);
  if (tid == 0) {
    t.hdr[H_M] = (!bad && v.method == 0 && cap > 0) ? m : 0;      // items the DP launches pass over
    t.hdr[H_STATUS] = bad; t.hdr[H_CAP] = cap; t.hdr[H_N] = n; t.hdr[H_LEN] = len; t.hdr[H_FRAMES] = n_frames; t.hdr[H_USERS] = n_users;
    t.hdr[H_METHOD] = v.method;
    a.status[vi] = bad;
  }
}

// item position j of every video's pass: grid (capacity chunks, videos).  The recurrence and the bit layout are sel_dp's (evalselect.hip).
__global__ __launch_bounds__(SL_DP_THREADS) void sel_long_dp_kernel(SelLongArgs a, int j) {
  const int vi = blockIdx.y;
  const SelLongTables t = sl_tables(a, vi);
  if (j >= t.hdr[H_M]) return;                                     // (0 for a nonzero status, method 1 and capacity 0)
  const int cap = t.hdr[H_CAP], c_base = blockIdx.x * SL_CHUNK;
  if (c_base > cap) return;
  const int w = t.swl[j], val = t.sv[j], words = (cap + 1 + 63) / 64;
  const int lane = threadIdx.x & 63;
  int* rows = (int*)(a.ws + (size_t)vi * a.pitch + a.rows_off);
  const int* __restrict__ prev = rows + (size_t)((j & 1) ^ 1) * (cap + 1);
  int* __restrict__ cur = rows + (size_t)(j & 1) * (cap + 1);
  unsigned long long* row = (unsigned long long*)(a.ws + (size_t)vi * a.pitch) + (size_t)j * words;
  for (int c0 = c_base + (threadIdx.x & ~63); c0 < c_base + SL_CHUNK && c0 <= cap; c0 += SL_DP_THREADS) {      // (a bound per wave: every lane reaches the ballot)
    const int c = c0 + lane;
    bool imp = false;
    if (c <= cap) {
      const int p = j > 0 ? prev[c] : 0;
      int best = p;
      if (c >= w) { const int cand = (j > 0 ? prev[c - w] : 0) + val; imp = cand > p; best = imp ? cand : p; }
      cur[c] = best;
    }
    const unsigned long long word = __ballot(imp);
    if (lane == 0) row[c0 >> 6] = word;
  }
}

// the selected set: grid (videos)
__global__ __launch_bounds__(SEL_THREADS) void sel_long_pick_kernel(SelLongArgs a) {
  __shared__ double s_x[SEL_MAX_SEGS];
  __shared__ int s_order[SEL_MAX_SEGS];
  __shared__ uint8_t s_sel[SEL_MAX_SEGS];
  const int vi = blockIdx.x, tid = threadIdx.x;
  const SelLongTables t = sl_tables(a, vi);
  const int bad = t.hdr[H_STATUS];
  if (bad == 4) return;
  const sumk_eval_dev_select v = a.vids[vi];
  const int n = t.hdr[H_N], cap = t.hdr[H_CAP];
  s_sel[tid] = 0;
  __syncthreads();
  if (!bad) {
    if (t.hdr[H_METHOD] == 0) {
      const unsigned long long* bits = (const unsigned long long*)(a.ws + (size_t)vi * a.pitch);
      if ((tid >> 6) == 0) sel_backtrack(bits, (cap + 1 + 63) / 64, n, cap, t.hdr[H_M], t.live, t.swl, t.w_all[0], s_sel);
    } else {
      sel_rank_walk(tid < n ? (double)v.seg_means[tid] : 0.0, n, cap, t.w_all, s_x, s_order, s_sel);
    }
  }
  __syncthreads();
  if (tid < n) a.selected[v.sel0 + tid] = s_sel[tid];              // (all zero for a video that was given up)
}

// the expanded summary and the partial counts of its chunk of frames: grid (frame chunks, videos)
__global__ __launch_bounds__(SL_FR_THREADS) void sel_long_expand_kernel(SelLongArgs a) {
  __shared__ int s_start[SEL_MAX_SEGS + 1];
  __shared__ uint8_t s_sel[SEL_MAX_SEGS];
  __shared__ int s_red[SL_FR_THREADS / 64][SL_SLOTS];
  const int vi = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SelLongTables t = sl_tables(a, vi);
  const int bad = t.hdr[H_STATUS];
  if (bad == 4) return;
  const sumk_eval_dev_select v = a.vids[vi];
  const int n = t.hdr[H_N], len = t.hdr[H_LEN], n_frames = t.hdr[H_FRAMES], n_users = t.hdr[H_USERS];
  for (int i = tid; i <= n; i += SL_FR_THREADS) s_start[i] = t.start[i];
  for (int i = tid; i < n; i += SL_FR_THREADS) s_sel[i] = bad ? 0 : a.selected[v.sel0 + i];
  __syncthreads();
  const bool count = !bad && n_users > 0;
  const long long range = count && n_frames > len ? n_frames : len;
  const long long per = (range + gridDim.x - 1) / gridDim.x, f_lo = blockIdx.x * per, f_hi = min(range, f_lo + per);
  float* out = a.summary + v.summary0;
  int gs[SEL_MAX_USERS], ov[SEL_MAX_USERS];
#pragma unroll
  for (int u = 0; u < SEL_MAX_USERS; ++u) { gs[u] = 0; ov[u] = 0; }
  int msum = 0;
  for (long long fl = f_lo + tid; fl < f_hi; fl += SL_FR_THREADS) {
    const int f = (int)fl;
    const int mi = (fl < len && s_sel[sel_segment_of(s_start, n, f)]) ? 1 : 0;
    if (fl < len) out[f] = mi ? 1.f : 0.f;
    if (count && f < n_frames) {
      msum += mi;
#pragma unroll
      for (int u = 0; u < SEL_MAX_USERS; ++u)
        if (u < n_users) {
          const int b = v.user_mask[(long long)u * n_frames + f] != 0 ? 1 : 0;
          gs[u] += b; ov[u] += b & mi;
        }
    }
  }
  if (!count) return;
  for (int u = 0; u <= n_users; ++u) {
    int g = msum, o = 0;
    if (u < n_users) {
#pragma unroll
      for (int q = 0; q < SEL_MAX_USERS; ++q) { g = q == u ? gs[q] : g; o = q == u ? ov[q] : o; }      // (a compile-time-unrollable select keeps them in registers)
    }
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) { g += __shfl_xor(g, mk, 64); o += __shfl_xor(o, mk, 64); }
    if (lane == 0) {
      if (u < n_users) { s_red[wave][2 * u] = g; s_red[wave][2 * u + 1] = o; }
      else s_red[wave][2 * SEL_MAX_USERS] = g;
    }
  }
  __syncthreads();
  int* part = (int*)(a.ws + (size_t)vi * a.pitch + a.counts_off) + (size_t)blockIdx.x * SL_SLOTS;
  for (int sl = tid; sl < SL_SLOTS; sl += SL_FR_THREADS) {
    if (sl < 2 * n_users || sl == 2 * SEL_MAX_USERS) {
      int c = 0;
      for (int q = 0; q < SL_FR_THREADS / 64; ++q) c += s_red[q][sl];
      part[sl] = c;
    }
  }
}

// the counts of the chunks added up, then the F-scores: grid (videos)
__global__ __launch_bounds__(64) void sel_long_fscores_kernel(SelLongArgs a, int n_chunks) {
  __shared__ int s_cnt[SL_SLOTS];
  __shared__ int s_gs[SEL_MAX_USERS], s_ov[SEL_MAX_USERS];
  __shared__ double s_f[SEL_MAX_USERS];
  const int vi = blockIdx.x, tid = threadIdx.x;
  const SelLongTables t = sl_tables(a, vi);
  const int bad = t.hdr[H_STATUS];
  if (bad == 4) return;                                            // (the prologue wrote its NaNs)
  const int n_users = t.hdr[H_USERS];
  if (bad || n_users == 0) {
    if (tid == 0) { a.f_avg[vi] = nan(""); a.f_max[vi] = nan(""); }
    return;
  }
  const int* part = (const int*)(a.ws + (size_t)vi * a.pitch + a.counts_off);
  for (int sl = tid; sl < SL_SLOTS; sl += 64) {
    int c = 0;
    if (sl < 2 * n_users || sl == 2 * SEL_MAX_USERS)
      for (int q = 0; q < n_chunks; ++q) c += part[(size_t)q * SL_SLOTS + sl];
    s_cnt[sl] = c;
  }
  __syncthreads();
  if (tid < n_users) { s_gs[tid] = s_cnt[2 * tid]; s_ov[tid] = s_cnt[2 * tid + 1]; }
  __syncthreads();
  if (tid == 0) {
    double fa, fm;
    if (t.hdr[H_LEN] >= t.hdr[H_FRAMES]) sel_fscores<float>(s_cnt[2 * SEL_MAX_USERS], s_ov, s_gs, n_users, 1e-8f, (float*)s_f, &fa, &fm);
    else sel_fscores<double>(s_cnt[2 * SEL_MAX_USERS], s_ov, s_gs, n_users, 1e-8, s_f, &fa, &fm);
    a.f_avg[vi] = fa; a.f_max[vi] = fm;
  }
}

}  // namespace sumk

using namespace sumk;

extern "C" int sumk_eval_device_segments_long(const float* scores_dev, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_video* videos_host,
                                              int32_t n_videos, float* frame_scratch_dev, float* seg_means_dev, void* stream) {
  SUMK_ARG(n_videos >= 0 && n_videos <= 65535, "eval_device_segments_long: n_videos=%d (at most 65535)", n_videos);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(scores_dev && videos_dev && videos_host && frame_scratch_dev && seg_means_dev, "eval_device_segments_long: null pointer");
  int max_frames = 0, max_segs = 0;
  for (int i = 0; i < n_videos; ++i) {
    const sumk_eval_dev_video& h = videos_host[i];
    SUMK_ARG(h.picks && (h.cps || h.n_segs == 0), "eval_device_segments_long: video %d has no picks / change points", i);
    SUMK_ARG(h.n_picks >= 1 && h.n_picks <= EL_MAX_PICKS, "eval_device_segments_long: video %d has %d picks (1 .. %d supported)", i, h.n_picks, EL_MAX_PICKS);
    SUMK_ARG(h.n_frames >= 1 && h.n_frames <= EL_MAX_FRAMES, "eval_device_segments_long: video %d has %d frames (1 .. %d supported)", i, h.n_frames, EL_MAX_FRAMES);
    SUMK_ARG(h.n_segs >= 0, "eval_device_segments_long: video %d has %d segments", i, h.n_segs);
    max_frames = h.n_frames > max_frames ? h.n_frames : max_frames; max_segs = h.n_segs > max_segs ? h.n_segs : max_segs;
  }
  hipLaunchKernelGGL(eval_upsample_long_kernel, dim3((max_frames + UP_CHUNK - 1) / UP_CHUNK, n_videos), dim3(UP_THREADS), 0, (hipStream_t)stream, scores_dev,
                     videos_dev, frame_scratch_dev);
  if (max_segs > 0)
    hipLaunchKernelGGL(eval_means_long_kernel, dim3(max_segs, n_videos), dim3(ML_THREADS), 0, (hipStream_t)stream, videos_dev, frame_scratch_dev, seg_means_dev);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" size_t sumk_eval_device_select_long_workspace_bytes(int32_t n_videos, int32_t max_n_segs, int32_t max_capacity) {
  if (n_videos < 1 || max_n_segs < 1 || max_n_segs > SEL_MAX_SEGS || max_capacity < 0 || max_capacity > SL_MAX_CAP) return 0;
  return (size_t)n_videos * sl_pitch(max_n_segs, max_capacity);
}

extern "C" int sumk_eval_device_select_long(const sumk_eval_dev_select* videos_dev, const sumk_eval_dev_select* videos_host, int32_t n_videos,
                                            float* machine_summary_dev, int64_t summary_total, uint8_t* selected_dev, int64_t selected_total,
                                            double* f_avg_dev, double* f_max_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  SUMK_ARG(n_videos >= 0 && n_videos <= 65535, "eval_device_select_long: n_videos=%d (at most 65535)", n_videos);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(videos_dev && videos_host && selected_dev && f_avg_dev && f_max_dev && status_dev && workspace, "eval_device_select_long: null pointer");
  SUMK_ARG(summary_total >= 0 && selected_total >= 0 && (machine_summary_dev || summary_total == 0), "eval_device_select_long: null summary");
  int max_segs = 0, max_cap = 0, max_frames = 0;
  int64_t max_range = 1;
  for (int i = 0; i < n_videos; ++i) {
    const sumk_eval_dev_select& h = videos_host[i];
    SUMK_ARG(h.seg_means && h.nfps, "eval_device_select_long: video %d has no segment means / nfps", i);
    SUMK_ARG(h.n_segs >= 1 && h.n_segs <= SEL_MAX_SEGS, "eval_device_select_long: video %d has %d segments (1 .. %d supported)", i, h.n_segs, SEL_MAX_SEGS);
    SUMK_ARG(h.capacity >= 0 && h.capacity <= SL_MAX_CAP, "eval_device_select_long: video %d has capacity %d (0 .. %d supported)", i, h.capacity, SL_MAX_CAP);
    SUMK_ARG(h.n_users >= 0 && h.n_users <= SEL_MAX_USERS, "eval_device_select_long: video %d has %d annotators (at most %d supported)", i, h.n_users, SEL_MAX_USERS);
    SUMK_ARG(h.n_frames >= 1 && h.n_frames <= SEL_MAX_FRAMES, "eval_device_select_long: video %d has %d frames (1 .. %d supported)", i, h.n_frames, SEL_MAX_FRAMES);
    SUMK_ARG(h.method == videos_host[0].method && (h.method == 0 || h.method == 1), "eval_device_select_long: method must be 0 (knapsack) or 1 (rank), one value per call");
    SUMK_ARG(h.summary_len >= 0 && h.summary0 >= 0 && h.summary0 + h.summary_len <= summary_total,
             "eval_device_select_long: video %d: summary [%lld, +%d) outside the %lld entries given", i, (long long)h.summary0, h.summary_len, (long long)summary_total);
    SUMK_ARG(h.sel0 >= 0 && h.sel0 + h.n_segs <= selected_total, "eval_device_select_long: video %d: segments [%lld, +%d) outside the %lld flags given", i,
             (long long)h.sel0, h.n_segs, (long long)selected_total);
    max_segs = h.n_segs > max_segs ? h.n_segs : max_segs; max_cap = h.capacity > max_cap ? h.capacity : max_cap;
    max_frames = h.n_frames > max_frames ? h.n_frames : max_frames;
    max_range = h.n_frames > max_range ? h.n_frames : max_range; max_range = h.summary_len > max_range ? h.summary_len : max_range;
  }
  const size_t need = (size_t)n_videos * sl_pitch(max_segs, max_cap);
  SUMK_ARG(workspace_bytes >= need, "eval_device_select_long: workspace %zu < required %zu", workspace_bytes, need);
  SUMK_ARG(((uintptr_t)workspace & 7) == 0, "eval_device_select_long: workspace must be 8-byte aligned");
  SelLongArgs a;
  a.vids = videos_dev; a.summary = machine_summary_dev; a.selected = selected_dev; a.f_avg = f_avg_dev; a.f_max = f_max_dev; a.status = status_dev;
  a.ws = (char*)workspace; a.pitch = sl_pitch(max_segs, max_cap);
  a.rows_off = sl_bits_bytes(max_segs, max_cap); a.items_off = a.rows_off + sl_rows_bytes(max_cap); a.counts_off = a.items_off + sl_items_bytes(max_segs);
  a.summary_total = summary_total; a.selected_total = selected_total; a.S = max_segs; a.max_cap = max_cap; a.max_frames = max_frames;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sel_long_prologue_kernel, dim3(n_videos), dim3(SEL_THREADS), 0, st, a);
  if (videos_host[0].method == 0 && max_cap > 0) {
    const dim3 grid(max_cap / SL_CHUNK + 1, n_videos);             // chunks of capacities 0 .. max_cap
    for (int j = 0; j < max_segs; ++j) hipLaunchKernelGGL(sel_long_dp_kernel, grid, dim3(SL_DP_THREADS), 0, st, a, j);
  }
  hipLaunchKernelGGL(sel_long_pick_kernel, dim3(n_videos), dim3(SEL_THREADS), 0, st, a);
  int64_t chunks = (max_range + SL_FR_PER_BLOCK - 1) / SL_FR_PER_BLOCK;
  const int n_chunks = (int)(chunks < 1 ? 1 : chunks > SL_FCHUNKS ? SL_FCHUNKS : chunks);
  hipLaunchKernelGGL(sel_long_expand_kernel, dim3(n_chunks, n_videos), dim3(SL_FR_THREADS), 0, st, a);
  hipLaunchKernelGGL(sel_long_fscores_kernel, dim3(n_videos), dim3(64), 0, st, a, n_chunks);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
