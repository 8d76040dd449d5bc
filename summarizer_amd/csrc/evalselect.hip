// Key-shot selection, summary expansion and F-scores on the device: the last step of the evaluation tail, behind the float32 segment
// means that sumk_eval_device_segments leaves in HBM (summarizer/utils/eval.py:74-165).  One launch per call, one workgroup per video,
// no atomics, no host synchronisation: the machine summary is a device tensor and the whole tail can be captured into a HIP graph.
// The specification is the host tail, bit for bit: eval_one / fscores of csrc/evaltail.hip and sumk_knapsack_dp of csrc/knapsack.hip.
//
//   values   (int64_t)((double)seg_mean * 1000.0), weights nfps[s]: the integers eval_one builds.
//   knapsack the host keeps, per capacity, the best profit and the LAST item that improved it (strict '>') and re-solves the shrinking
//            sub-problem (items < s, capacity rem) once per selected item.  The `last` array of that sub-problem IS the state of
//            last[0 .. rem] after the first s items of the one full pass (the DP at capacity c reads capacities <= c only), so ONE
//            pass suffices when it records, per (item, capacity), whether the item improved the capacity: one bit per pair, in the
//            caller's workspace.  Backtrack from (k = n, rem = capacity): s = the largest item < k whose bit is set at rem, item 0 if
//            there is none; rem -= w[s]; k = s; s is selected if rem >= 0; repeat while rem > 0 and k > 0.  For one item all
//            capacities are independent given the previous row (cand = prev[c - w] + v): threads stride over c on two rows, one
//            barrier per item.  An item with w > capacity or v <= 0 never improves a capacity (profits are non-decreasing in c): such
//            items are left out of the pass altogether, which is what makes the empty pad segments of sumk_kts_segments free.
//            Rows are int32 (the kernel checks that the values of the items in the pass sum below 2^31: the result is then the
//            int64 host's), in LDS up to capacity 4095, in the workspace above.
//   rank     eval_one's stable_sort by ascending double score walked from the back = descending score, the larger index first among
//            equals; sorted position by counting in LDS, the greedy walk (strict total + nfps < capacity) on one thread.
//   F-scores fscores<float> when summary_len >= n_frames (truncation), fscores<double> when shorter (zero padding); the sums are
//            counts of 0/1 and exact in any order, the `+ 1e-8` steps keep the host's types, the mean over annotators is numpy's
//            pairwise tree.  This unit is compiled without FMA contraction, like evaldev.hip.
#include "evaldev_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace sumk {

namespace {
constexpr int SEL_MAX_CAP = SUMK_SELECT_MAX_CAPACITY;
constexpr int SEL_LDS_CAP = SUMK_SELECT_LDS_CAPACITY;        // two int32 rows of SEL_LDS_CAP + 1 entries: 32 KiB
// (SEL_THREADS, SEL_MAX_SEGS, SEL_MAX_USERS and SEL_MAX_FRAMES -- 16 bits hold a thread's share of 2^24 frames -- are in evaldev_common.h)

inline size_t sel_words(int64_t capacity) { return (size_t)((capacity + 1 + 63) / 64); }
inline size_t sel_bits_bytes(int max_segs, int max_cap) { return align_up((size_t)max_segs * sel_words(max_cap) * 8, 256); }
inline size_t sel_pitch(int max_segs, int max_cap) {
  return sel_bits_bytes(max_segs, max_cap) + (max_cap > SEL_LDS_CAP ? align_up(2 * ((size_t)max_cap + 1) * 4, 256) : 0);
}
}  // namespace

struct SelArgs {
  const sumk_eval_dev_select* vids;
  float* summary; uint8_t* selected; double* f_avg; double* f_max; int32_t* status;
  char* ws; size_t pitch, bits_bytes;      // per video: improvement bits, then (capacity > SEL_LDS_CAP) the two profit rows
};

// (sel_scan, sel_prepare, sel_segment_of, sel_backtrack and sel_rank_walk are in evaldev_common.h: evallong.hip takes the same steps)

// The one pass of the DP over the m items it keeps (values sv, weights swl, by position), rows r0 / r1 both in LDS or both in the
// workspace (one inlined copy per address space); bit (j, c) of `bits` = item j improved capacity c.  Ends on a barrier.
__device__ __forceinline__ void sel_dp(int* r0, int* r1, unsigned long long* __restrict__ bits, const int* sv, const int* swl, int m, int cap,
                                       int words) {
  const int tid = threadIdx.x;
  for (int c = tid; c <= cap; c += SEL_THREADS) r0[c] = 0;
  __syncthreads();
  int* prev = r0; int* cur = r1;
  for (int j = 0; j < m; ++j) {
    const int w = swl[j], v = sv[j];
    unsigned long long* row = bits + (size_t)j * words;
    for (int c0 = (tid & ~63); c0 <= cap; c0 += SEL_THREADS) {            // (a bound per wave: every lane of a wave reaches the ballot)
      const int c = c0 + (tid & 63);
      bool imp = false;
      if (c <= cap) {
        const int p = prev[c];
        int best = p;
        if (c >= w) { const int cand = prev[c - w] + v; imp = cand > p; best = imp ? cand : p; }
        cur[c] = best;
      }
      const unsigned long long word = __ballot(imp);
      if ((tid & 63) == 0) row[c0 >> 6] = word;
    }
    __syncthreads();
    int* t = prev; prev = cur; cur = t;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void eval_select_kernel(SelArgs a) {
  __shared__ __attribute__((aligned(16))) int s_rows[2 * (SEL_LDS_CAP + 1)];      // knapsack: two profit rows; rank: scores + order
  __shared__ int s_v[SEL_MAX_SEGS], s_wl[SEL_MAX_SEGS];                           // value / weight of the items in the pass, by position
  __shared__ int s_w[SEL_MAX_SEGS];                                               // weight of every segment
  __shared__ int s_start[SEL_MAX_SEGS + 1];                                       // prefix sum of nfps
  __shared__ uint16_t s_live[SEL_MAX_SEGS];                                       // segment of the item at a position
  __shared__ uint8_t s_sel[SEL_MAX_SEGS];
  __shared__ long long s_wsum[SEL_WAVES];
  __shared__ int s_flag[2];
  __shared__ int s_red[SEL_WAVES][2 * SEL_MAX_USERS + 1];
  __shared__ double s_f[SEL_MAX_USERS];
  const int vi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const sumk_eval_dev_select v = a.vids[vi];
  const int n = v.n_segs, cap = v.capacity, len = v.summary_len, n_frames = v.n_frames;
  const int n_users = (v.user_mask != nullptr && v.n_users > 0) ? v.n_users : 0;
  // the entry point checked the host copy of the descriptors; a device copy that disagrees with it must still write nothing out of bounds
  if (n < 1 || n > SEL_MAX_SEGS || cap < 0 || cap > SEL_MAX_CAP || n_users > SEL_MAX_USERS || len < 0 || n_frames < 1 ||
      n_frames > SEL_MAX_FRAMES || (v.method != 0 && v.method != 1) || v.seg_means == nullptr || v.nfps == nullptr) {
    if (tid == 0) { a.status[vi] = 4; a.f_avg[vi] = nan(""); a.f_max[vi] = nan(""); }
    return;
  }
  s_sel[tid] = 0;
  int m; double x;
  const int bad = sel_prepare(v, n, cap, len, s_flag, s_wsum, s_w, s_start, s_live, s_v, s_wl, &m, &x);
  if (!bad) {
    if (v.method == 0) {
      unsigned long long* bits = (unsigned long long*)(a.ws + (size_t)vi * a.pitch);
      const int words = (cap + 1 + 63) / 64;
      if (cap > 0 && m > 0) {
        if (cap <= SEL_LDS_CAP) {
          sel_dp(s_rows, s_rows + (cap + 1), bits, s_v, s_wl, m, cap, words);
        } else {
          int* r0 = (int*)(a.ws + (size_t)vi * a.pitch + a.bits_bytes);
          sel_dp(r0, r0 + (cap + 1), bits, s_v, s_wl, m, cap, words);
        }
      }
      if (wave == 0) sel_backtrack(bits, words, n, cap, cap > 0 ? m : 0, s_live, s_wl, s_w[0], s_sel);
    } else {
      double* s_x = (double*)s_rows;
      int* s_order = (int*)(s_x + SEL_MAX_SEGS);
      sel_rank_walk(x, n, cap, s_w, s_x, s_order, s_sel);
    }
  }
  __syncthreads();
  // ---- selected flags and the expanded summary (all zero for a video that was given up)
  if (tid < n) a.selected[v.sel0 + tid] = s_sel[tid];
  float* out = a.summary + v.summary0;
  for (int f = tid; f < len; f += SEL_THREADS) out[f] = (!bad && s_sel[sel_segment_of(s_start, n, f)]) ? 1.f : 0.f;
  if (tid == 0) a.status[vi] = bad;
  if (bad || n_users == 0) {
    if (tid == 0) { a.f_avg[vi] = nan(""); a.f_max[vi] = nan(""); }
    return;
  }
  // ---- F-scores: per annotator the overlap with the machine summary and the annotator's own count, 16 bits each per thread
  const int lim = len < n_frames ? len : n_frames;
  int acc[SEL_MAX_USERS];
#pragma unroll
  for (int u = 0; u < SEL_MAX_USERS; ++u) acc[u] = 0;
  int msum = 0;
  for (int f = tid; f < n_frames; f += SEL_THREADS) {
    const int mi = (f < lim && s_sel[sel_segment_of(s_start, n, f)]) ? 1 : 0;
    msum += mi;
#pragma unroll
    for (int u = 0; u < SEL_MAX_USERS; ++u)
      if (u < n_users) {
        const int b = v.user_mask[(long long)u * n_frames + f] != 0 ? 1 : 0;
        acc[u] += b + ((b & mi) << 16);
      }
  }
  for (int u = 0; u <= n_users; ++u) {
    int p = 0;
#pragma unroll
    for (int q = 0; q < SEL_MAX_USERS; ++q) p = q == u ? acc[q] : p;      // (a compile-time-unrollable select keeps acc in registers)
    int g = u < n_users ? (p & 0xffff) : msum, o = u < n_users ? (p >> 16) : 0;
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) { g += __shfl_xor(g, mk, 64); o += __shfl_xor(o, mk, 64); }
    if (lane == 0) {
      if (u < n_users) { s_red[wave][2 * u] = g; s_red[wave][2 * u + 1] = o; }
      else s_red[wave][2 * SEL_MAX_USERS] = g;
    }
  }
  __syncthreads();
  int* s_gs = s_rows; int* s_ov = s_rows + SEL_MAX_USERS;                  // (the profit rows are free by now)
  if (tid < n_users) {
    int g = 0, o = 0;
    for (int q = 0; q < SEL_WAVES; ++q) { g += s_red[q][2 * tid]; o += s_red[q][2 * tid + 1]; }
    s_gs[tid] = g; s_ov[tid] = o;
  }
  __syncthreads();
  if (tid == 0) {
    int ms = 0;
    for (int q = 0; q < SEL_WAVES; ++q) ms += s_red[q][2 * SEL_MAX_USERS];
    double fa, fm;
    if (len >= n_frames) sel_fscores<float>(ms, s_ov, s_gs, n_users, 1e-8f, (float*)s_f, &fa, &fm);
    else sel_fscores<double>(ms, s_ov, s_gs, n_users, 1e-8, s_f, &fa, &fm);
    a.f_avg[vi] = fa; a.f_max[vi] = fm;
  }
}

// ---- sumk_kts_segments: (n_cps, cps) of sumk_kts -> the (change_points, n_frame_per_seg) layout the tail reads, at a fixed pitch of
// max_ncp + 1 segments per video; live segments as utils.kts.cps_to_segments, the rest EMPTY: (n_frames, n_frames - 1), nfps 0.
__global__ __launch_bounds__(256) void kts_segments_kernel(const int32_t* __restrict__ n_cps, const int32_t* __restrict__ cps, int max_ncp,
                                                           const int32_t* __restrict__ off, const int32_t* const* __restrict__ picks,
                                                           const int32_t* __restrict__ n_frames, int32_t* __restrict__ change_points,
                                                           int32_t* __restrict__ nfps) {
  const int v = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x, pitch = max_ncp + 1;
  if (s >= pitch) return;
  const int n = off[v + 1] - off[v], nf = n_frames[v];
  int m = n_cps[v];
  m = m < 0 ? 0 : m > max_ncp ? max_ncp : m;
  const int32_t* pk = picks != nullptr ? picks[v] : nullptr;
  const int32_t* c = cps + (int64_t)v * max_ncp;
  auto frame_of = [&](int k) {                // the frame at which change point k starts a segment
    int step = c[k];
    step = step < 0 ? 0 : step > n - 1 ? n - 1 : step;
    return pk != nullptr ? pk[step] : step;
  };
  int lo = nf, hi = nf - 1;
  if (s <= m) {
    lo = s == 0 ? 0 : frame_of(s - 1);
    hi = s == m ? nf - 1 : frame_of(s) - 1;
  }
  const int64_t at = (int64_t)v * pitch + s;
  change_points[2 * at] = lo; change_points[2 * at + 1] = hi;
  nfps[at] = hi - lo + 1;
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_eval_device_select_workspace_bytes(int32_t n_videos, int32_t max_n_segs, int32_t max_capacity) {
  if (n_videos < 1 || max_n_segs < 1 || max_n_segs > SEL_MAX_SEGS || max_capacity < 0 || max_capacity > SEL_MAX_CAP) return 0;
  return (size_t)n_videos * sel_pitch(max_n_segs, max_capacity);
}

extern "C" int sumk_eval_device_select(const sumk_eval_dev_select* videos_dev, const sumk_eval_dev_select* videos_host, int32_t n_videos,
                                       float* machine_summary_dev, int64_t summary_total, uint8_t* selected_dev, int64_t selected_total,
                                       double* f_avg_dev, double* f_max_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  SUMK_ARG(n_videos >= 0, "eval_device_select: n_videos=%d", n_videos);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(videos_dev && videos_host && selected_dev && f_avg_dev && f_max_dev && status_dev && workspace, "eval_device_select: null pointer");
  SUMK_ARG(summary_total >= 0 && selected_total >= 0 && (machine_summary_dev || summary_total == 0), "eval_device_select: null summary");
  int max_segs = 0, max_cap = 0;
  for (int i = 0; i < n_videos; ++i) {
    const sumk_eval_dev_select& h = videos_host[i];
    SUMK_ARG(h.seg_means && h.nfps, "eval_device_select: video %d has no segment means / nfps", i);
    SUMK_ARG(h.n_segs >= 1 && h.n_segs <= SEL_MAX_SEGS, "eval_device_select: video %d has %d segments (1 .. %d supported)", i, h.n_segs, SEL_MAX_SEGS);
    SUMK_ARG(h.capacity >= 0 && h.capacity <= SEL_MAX_CAP, "eval_device_select: video %d has capacity %d (0 .. %d supported)", i, h.capacity, SEL_MAX_CAP);
    SUMK_ARG(h.n_users >= 0 && h.n_users <= SEL_MAX_USERS, "eval_device_select: video %d has %d annotators (at most %d supported)", i, h.n_users, SEL_MAX_USERS);
    SUMK_ARG(h.n_frames >= 1 && h.n_frames <= SEL_MAX_FRAMES, "eval_device_select: video %d has %d frames (1 .. %d supported)", i, h.n_frames, SEL_MAX_FRAMES);
    SUMK_ARG(h.method == videos_host[0].method && (h.method == 0 || h.method == 1), "eval_device_select: method must be 0 (knapsack) or 1 (rank), one value per call");
    SUMK_ARG(h.summary_len >= 0 && h.summary0 >= 0 && h.summary0 + h.summary_len <= summary_total,
             "eval_device_select: video %d: summary [%lld, +%d) outside the %lld entries given", i, (long long)h.summary0, h.summary_len, (long long)summary_total);
    SUMK_ARG(h.sel0 >= 0 && h.sel0 + h.n_segs <= selected_total, "eval_device_select: video %d: segments [%lld, +%d) outside the %lld flags given", i,
             (long long)h.sel0, h.n_segs, (long long)selected_total);
    max_segs = h.n_segs > max_segs ? h.n_segs : max_segs; max_cap = h.capacity > max_cap ? h.capacity : max_cap;
  }
  const size_t need = (size_t)n_videos * sel_pitch(max_segs, max_cap);
  SUMK_ARG(workspace_bytes >= need, "eval_device_select: workspace %zu < required %zu", workspace_bytes, need);
  SUMK_ARG(((uintptr_t)workspace & 7) == 0, "eval_device_select: workspace must be 8-byte aligned");
  SelArgs a;
  a.vids = videos_dev; a.summary = machine_summary_dev; a.selected = selected_dev; a.f_avg = f_avg_dev; a.f_max = f_max_dev; a.status = status_dev;
  a.ws = (char*)workspace; a.pitch = sel_pitch(max_segs, max_cap); a.bits_bytes = sel_bits_bytes(max_segs, max_cap);
  hipLaunchKernelGGL(eval_select_kernel, dim3(n_videos), dim3(SEL_THREADS), 0, (hipStream_t)stream, a);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_kts_segments(const int32_t* n_cps_dev, const int32_t* cps_dev, int32_t n_seq, int32_t max_ncp, const int32_t* seq_off_dev,
                                 const int32_t* const* picks_dev, const int32_t* n_frames_dev, int32_t* change_points_dev, int32_t* nfps_dev,
                                 void* stream) {
  SUMK_ARG(n_seq >= 0 && max_ncp >= 0, "kts_segments: n_seq=%d max_ncp=%d", n_seq, max_ncp);
  if (n_seq == 0) return SUMK_OK;
  SUMK_ARG(n_cps_dev && (cps_dev || max_ncp == 0) && seq_off_dev && n_frames_dev && change_points_dev && nfps_dev, "kts_segments: null pointer");
  hipLaunchKernelGGL(kts_segments_kernel, dim3((max_ncp + 1 + 255) / 256, n_seq), dim3(256), 0, (hipStream_t)stream, n_cps_dev, cps_dev, max_ncp,
                     seq_off_dev, picks_dev, n_frames_dev, change_points_dev, nfps_dev);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
