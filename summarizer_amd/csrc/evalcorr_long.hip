// Rank correlation on the device evaluation tail for long videos: sumk_eval_device_spearman_long and sumk_eval_device_kendall_long take the
// place of sumk_eval_device_spearman (evaldev.hip: pick intervals in LDS, 4096 at most, ranked by an O(groups^2) count) and
// sumk_eval_device_kendall (evalkendall.hip: a video's frame keys sorted in LDS, 16 384 at most) for what sumk_eval_device_segments_long
// and sumk_eval_device_select_long accept.  The descriptors, the results and the rules are those kernels'; the tables live in the workspace.
//
//   sort       ONE building block serves the three sorts below: a chip-wide stable merge sort.  Workgroups sort tiles of SUMK_CORR_LONG_TILE
//              keys in LDS with the scheme of kd_merge_sort (evaldev_common.h), then one launch per merge level over two buffers of the
//              workspace (ping-pong).  At each level every element finds its place by one binary search in the sibling run -- lower bound
//              for an element of a left run, upper bound for one of a right run, kd_merge_sort's rule: stable -- and an element of a left
//              run adds its search result to an inversion count (an integer atomic).  Templated on the key type (32 / 64 bit), on whose
//              arrays it sorts (the groups of a video, the frames of a (video, annotator)) and on "count inversions".  Grids are over
//              (chunks, annotators, videos); a block past its array's length exits at once.
//   groups     a video's groups are its pick intervals plus the frames no interval covers (value 0): interval i = [max(0, picks[i]),
//              min(n_frames, picks[i + 1] or n_frames)) with value scores[row0 + i] for i < n_steps, else 0 (ed_intervals).  The keys
//              kendall_float_key(value) << 32 | group are sorted; an inclusive prefix sum P of the groups' frame counts in sorted order and
//              one of the "new key" flags (three launches: block sums, their scan, the scan inside the blocks) give all the tie arithmetic:
//              with [lo, hi) the positions that hold a group's key, equal = P[hi] - P[lo] and greater = n_frames - P[hi], integers.
//   Spearman   rank of a group = greater + 0.5 (equal + 1) -- the values eval_spearman_part_kernel counts; smm = sum over GROUPS of
//              frames (rank - mean)^2; the cross terms run over (frame chunks, videos), the group of a frame by binary search in the picks.
//              A video of n frames is cut into min(256, ceil(n / 4096)) chunks, whatever else the call holds; a last launch adds the
//              partial sums in chunk order.
//   Kendall    the steps of evalkendall.hip's header comment in global memory: dense x rank of a group = distinct keys below it; xtie from
//              the groups; frame key = x rank << 24 | y_dense (64 bit), sorted; runs of equal keys give ntie (a run's head finds its end by one
//              upper-bound search); the y parts in (x, y) order, sorted with the inversion count on, give dis.  kendall_tau_b, then the mean
//              over annotators in numpy's order.
// No cooperative launch, no flag polled across workgroups: every launch ends by itself and the launches depend on the host copy of the
// descriptors only (a call captures into a HIP graph).  No float atomics; float64 partial sums are added in a fixed order.  Compiled
// without FMA contraction, like evalkendall.hip.
#include "evaldev_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace sumk {

namespace {
constexpr int CL_MAX_PICKS = SUMK_SEGMENTS_LONG_MAX_PICKS;
constexpr int CL_MAX_FRAMES = SUMK_SEGMENTS_LONG_MAX_FRAMES;
constexpr int CL_TILE = SUMK_CORR_LONG_TILE;
constexpr int CL_SORT_THREADS = 512;
constexpr int CL_THREADS = 256;
constexpr int CL_MERGE_PER_THREAD = 4, CL_MERGE_BLOCK = CL_THREADS * CL_MERGE_PER_THREAD;      // keys per block of a merge level
constexpr int CL_SCAN_PER_THREAD = 4, CL_SCAN_BLOCK = CL_THREADS * CL_SCAN_PER_THREAD;      // sorted groups per scan block
constexpr int CL_CHUNK_FRAMES = 4096, CL_MAX_CHUNKS = 256;                                    // Spearman: frames per chunk, chunks per video at most
constexpr int CL_SLOTS = ED_MAX_USERS + 1;                                                    // per chunk: a cross term per annotator, then smm
constexpr int CL_Y_BITS = 24;                                                                 // a dense annotator rank: < n_frames <= 2^24
static_assert((CL_TILE & (CL_TILE - 1)) == 0 && CL_TILE % CL_SORT_THREADS == 0 && 2 * CL_TILE * 8 <= 64 * 1024, "a tile and its ping-pong copy fit static LDS");
static_assert(CL_MAX_FRAMES <= (1 << CL_Y_BITS) && CL_MAX_PICKS + 1 < (1 << 21), "frame key = x rank << 24 | y rank");

typedef unsigned long long u64;

// what the prologue leaves per video: where its tables start and what the later launches go by.  bad: 0 fine; 1 a device descriptor past
// the limits or past what the host copy sized the workspace and the grids for (NaN, Kendall: -1 counts); 2 no annotators (NaN)
struct ClHdr {
  long long g_off, sb_off, uf_off, part_off, u_off;      // first group / scan block / (annotator, frame) / chunk / annotator slot
  int bad, n_int, n_grp, n_frames, n_users, n_chunks, uncovered, pad_;
};

struct ClLayout {
  long long total_g, total_sb, total_uf, total_part, total_users;
  int max_grp, max_frames, max_users, max_chunks;
  size_t hdr, ga, gb, gp, gd, gbs, rank, part, xr, fa, fb, ctr, total;      // byte offsets of the parts, then the size
};

struct ClArgs {
  const float* scores; const sumk_eval_dev_video* vids; const sumk_eval_dev_kendall* kds;
  ClHdr* hdr; u64* ga; u64* gb; int* gp; int* gd; long long* gbs; double* rank; double* part; int* xr; u64* fa; u64* fb; u64* ctr;
  long long total_g, total_sb, total_uf, total_part, total_users;
  int n_videos, max_grp, max_frames, max_users, kendall;
};

__host__ __device__ inline int cl_chunks(int n_frames) {
  const int c = (n_frames + CL_CHUNK_FRAMES - 1) / CL_CHUNK_FRAMES;
  return c < 1 ? 1 : c > CL_MAX_CHUNKS ? CL_MAX_CHUNKS : c;
}

// the parts of the workspace from the host copy of the descriptors; false: a video past a limit
bool cl_layout(const sumk_eval_dev_video* h, int n, bool kendall, ClLayout* L) {
  *L = ClLayout();
  if (h == nullptr || n < 1 || n > 65535) return false;
  for (int i = 0; i < n; ++i) {
    if (h[i].n_picks < 1 || h[i].n_picks > CL_MAX_PICKS || h[i].n_frames < 1 || h[i].n_frames > CL_MAX_FRAMES || h[i].n_users > ED_MAX_USERS) return false;
    const int grp = h[i].n_picks + 1, nu = h[i].n_users > 0 ? h[i].n_users : 0, nc = kendall ? 0 : cl_chunks(h[i].n_frames);
    L->total_g += grp; L->total_sb += (grp + CL_SCAN_BLOCK - 1) / CL_SCAN_BLOCK; L->total_users += nu;
    L->total_uf += kendall ? (long long)nu * h[i].n_frames : 0; L->total_part += nc;
    L->max_grp = grp > L->max_grp ? grp : L->max_grp; L->max_frames = h[i].n_frames > L->max_frames ? h[i].n_frames : L->max_frames;
    L->max_users = nu > L->max_users ? nu : L->max_users; L->max_chunks = nc > L->max_chunks ? nc : L->max_chunks;
  }
  size_t at = 0;
  auto part = [&at](size_t bytes) { const size_t o = at; at += align_up(bytes, 256); return o; };
  L->hdr = part((size_t)n * sizeof(ClHdr));
  L->ga = part((size_t)L->total_g * 8); L->gb = part((size_t)L->total_g * 8);
  L->gp = part((size_t)L->total_g * 4); L->gd = part((size_t)L->total_g * 4); L->gbs = part((size_t)L->total_sb * 8);
  if (!kendall) {
    L->rank = part((size_t)L->total_g * 8); L->part = part((size_t)L->total_part * CL_SLOTS * 8);
  } else {
    L->xr = part((size_t)L->total_g * 4); L->fa = part((size_t)L->total_uf * 8); L->fb = part((size_t)L->total_uf * 8);
    L->ctr = part(((size_t)2 * L->total_users + n) * 8);
  }
  L->total = at;
  return true;
}

ClArgs cl_args(const ClLayout& L, char* ws, const float* scores, const sumk_eval_dev_video* vids, const sumk_eval_dev_kendall* kds, int n, bool kendall) {
  ClArgs a;
  a.scores = scores; a.vids = vids; a.kds = kds;
  a.hdr = (ClHdr*)(ws + L.hdr); a.ga = (u64*)(ws + L.ga); a.gb = (u64*)(ws + L.gb); a.gp = (int*)(ws + L.gp); a.gd = (int*)(ws + L.gd);
  a.gbs = (long long*)(ws + L.gbs); a.rank = (double*)(ws + L.rank); a.part = (double*)(ws + L.part); a.xr = (int*)(ws + L.xr);
  a.fa = (u64*)(ws + L.fa); a.fb = (u64*)(ws + L.fb); a.ctr = (u64*)(ws + L.ctr);
  a.total_g = L.total_g; a.total_sb = L.total_sb; a.total_uf = L.total_uf; a.total_part = L.total_part; a.total_users = L.total_users;
  a.n_videos = n; a.max_grp = L.max_grp; a.max_frames = L.max_frames; a.max_users = L.max_users; a.kendall = kendall ? 1 : 0;
  return a;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ prologue
// One thread walks the videos: the entry point checked the host copy of the descriptors and sized the workspace and the grids by it; a
// device copy that disagrees with it and is past a limit, past the call's largest sizes or past what is left of a part is marked bad and
// takes no room.  Nothing later reads or writes outside what is handed out here.
__global__ __launch_bounds__(64) void cl_prologue_kernel(ClArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long g = 0, sb = 0, uf = 0, pt = 0, us = 0;
  for (int vi = 0; vi < a.n_videos; ++vi) {
    const sumk_eval_dev_video d = a.vids[vi];
    ClHdr h;
    h.g_off = g; h.sb_off = sb; h.uf_off = uf; h.part_off = pt; h.u_off = us;
    h.bad = 1; h.n_int = 0; h.n_grp = 0; h.n_frames = d.n_frames; h.n_users = d.n_users; h.n_chunks = 0; h.uncovered = 0; h.pad_ = 0;
    const int nu = d.n_users > 0 ? d.n_users : 0;
    bool ok = d.picks != nullptr && d.n_picks >= 1 && d.n_picks <= CL_MAX_PICKS && d.n_picks + 1 <= a.max_grp && d.n_frames >= 1 &&
              d.n_frames <= CL_MAX_FRAMES && d.n_frames <= a.max_frames && d.n_users <= ED_MAX_USERS && nu <= a.max_users;
    if (ok) {
      const long long grp = d.n_picks + 1, nsb = (grp + CL_SCAN_BLOCK - 1) / CL_SCAN_BLOCK, nuf = a.kendall ? (long long)nu * d.n_frames : 0;
      const int nc = a.kendall ? 0 : cl_chunks(d.n_frames);
      ok = g + grp <= a.total_g && sb + nsb <= a.total_sb && uf + nuf <= a.total_uf && pt + nc <= a.total_part && us + nu <= a.total_users;
      if (ok && a.kendall && nu > 0) ok = a.kds[vi].y_dense != nullptr && a.kds[vi].ytie != nullptr;
      if (ok && !a.kendall && nu > 0 && d.user_ranks != nullptr) ok = d.user_mean != nullptr && d.user_ssq != nullptr;
      if (ok) {
        const bool sentinel = d.picks[d.n_picks - 1] != d.n_frames;
        h.n_int = d.n_picks - 1 + (sentinel ? 1 : 0);
        h.n_grp = h.n_int + 1;
        h.n_chunks = nc;
        // picks ascend (the caller's promise), so the intervals tile [max(0, picks[0]), n_frames): the frames in front are the uncovered ones
        h.uncovered = min(d.n_frames, max(0, d.picks[0]));
        h.bad = (nu == 0 || (!a.kendall && d.user_ranks == nullptr)) ? 2 : 0;
        g += grp; sb += nsb; uf += nuf; pt += nc; us += nu;
      }
    }
    a.hdr[vi] = h;
  }
}

// the integer counters of a Kendall call start at zero (a launch of its own: a kernel node like the others when the call is captured)
__global__ __launch_bounds__(CL_THREADS) void cl_zero_kernel(u64* __restrict__ p, long long n) {
  const long long i = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i < n) p[i] = 0;
}

// ------------------------------------------------------------------------------------------------ groups
// frames of group g: an interval's length, or (g == n_int) the frames no interval covers
__device__ __forceinline__ int cl_group_frames(const sumk_eval_dev_video& v, const ClHdr& h, int g) {
  if (g >= h.n_int) return h.uncovered;
  const int lo = max(0, v.picks[g]), hi = min(h.n_frames, g + 1 < v.n_picks ? v.picks[g + 1] : h.n_frames);
  return max(0, hi - lo);
}
// the group of frame f: the last interval that starts at or in front of f (empty intervals of repeated picks are passed over), or the
// uncovered group when f lies in front of the first pick -- the upsample rule of eval_upsample_long_kernel
__device__ __forceinline__ int cl_group_of(const int32_t* __restrict__ picks, int n_int, int f) {
  int lo = 0, hi = n_int;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (picks[m] <= f) lo = m + 1; else hi = m; }
  return lo > 0 ? lo - 1 : n_int;
}

// grid (group chunks, videos)
__global__ __launch_bounds__(CL_THREADS) void cl_group_keys_kernel(ClArgs a) {
  const ClHdr h = a.hdr[blockIdx.y];
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (h.bad || i >= h.n_grp) return;
  const sumk_eval_dev_video v = a.vids[blockIdx.y];
  const float val = (i < h.n_int && i < v.n_steps) ? a.scores[v.row0 + i] : 0.f;
  a.ga[h.g_off + i] = ((u64)kendall_float_key(val) << 32) | (u64)(uint32_t)i;
}

// ------------------------------------------------------------------------------------------------ the sort
// elements of the sorted run a[0..n) whose upper bits (>> SH) are below those of v / not above them
template <int SH, class K>
__device__ __forceinline__ int cl_lower(const K* a, int n, K v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if ((a[m] >> SH) < (v >> SH)) lo = m + 1; else hi = m; }
  return lo;
}
template <int SH, class K>
__device__ __forceinline__ int cl_upper(const K* a, int n, K v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if ((a[m] >> SH) <= (v >> SH)) lo = m + 1; else hi = m; }
  return lo;
}

// The array a block sorts and its other buffer.  64-bit keys: the same offset in the two buffers a0 / b0; FR: the frames of (video,
// annotator u), else the groups of the video.  32-bit keys (the y parts of a (video, annotator)): the two halves of the 8 n bytes the pair
// owns in a0.  false: nothing to sort here.
template <class K, bool FR>
__device__ __forceinline__ bool cl_seg(const ClHdr& h, int u, K* a0, K* b0, K** a, K** b, int* n) {
  if (h.bad) return false;
  if (FR) {
    if (u >= h.n_users) return false;
    const long long off = h.uf_off + (long long)u * h.n_frames;
    *n = h.n_frames;
    if (sizeof(K) == 4) { *a = a0 + 2 * off; *b = *a + h.n_frames; }
    else { *a = a0 + off; *b = b0 + off; }
  } else {
    if (u != 0) return false;
    *n = h.n_grp; *a = a0 + h.g_off; *b = b0 + h.g_off;
  }
  return true;
}

// the block's count to a counter of the workspace, ONE atomic per block (every block of a (video, annotator) adds to the same word: an
// atomic per wave kept the merge levels of a long video waiting on that word -- DESIGN.md).  Integers: any order gives the same sum.
// Every thread of the block of NT threads calls it (a barrier inside).
template <int NT>
__device__ __forceinline__ void cl_add_block(u64* dst, long long x) {
  __shared__ long long s_cnt[NT / 64];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t = 0;
    for (int w = 0; w < NT / 64; ++w) t += s_cnt[w];
    if (t != 0) atomicAdd(dst, (u64)t);
  }
}

// tiles of CL_TILE keys, sorted where they lie: grid (tiles, annotators | 1, videos)
template <class K, bool FR, bool INV>
__global__ __launch_bounds__(CL_SORT_THREADS) void cl_tile_sort_kernel(const ClHdr* __restrict__ hdr, K* a0, K* b0, u64* ctr) {
  __shared__ K s_a[CL_TILE], s_b[CL_TILE];
  const ClHdr h = hdr[blockIdx.z];
  K *ga, *gb; int n;
  if (!cl_seg<K, FR>(h, blockIdx.y, a0, b0, &ga, &gb, &n)) return;
  const int base = blockIdx.x * CL_TILE;
  if (base >= n) return;
  const int m = min(CL_TILE, n - base), tid = threadIdx.x;
  for (int i = tid; i < m; i += CL_SORT_THREADS) s_a[i] = ga[base + i];
  __syncthreads();
  K *x = s_a, *y = s_b;
  long long inv = 0;
  for (int w = 1; w < m; w <<= 1) {
    for (int i = tid; i < m; i += CL_SORT_THREADS) {
      const int s = i & ~(2 * w - 1), mid = min(s + w, m), end = min(s + 2 * w, m);
      const K v = x[i];
      int dst;
      if (i < mid) {
        const int c = cl_lower<0>(x + mid, end - mid, v);      // right-run elements below v: they overtake it
        inv += c;
        dst = i + c;
      } else {
        dst = s + (i - mid) + cl_upper<0>(x + s, mid - s, v);   // left-run elements not above v stay in front
      }
      y[dst] = v;
    }
    __syncthreads();
    K* t = x; x = y; y = t;
  }
  for (int i = tid; i < m; i += CL_SORT_THREADS) ga[base + i] = x[i];
  if (INV) cl_add_block<CL_SORT_THREADS>(ctr + 2 * (h.u_off + blockIdx.y) + 1, inv);
}

// one merge level, runs of w keys: grid (chunks of CL_MERGE_BLOCK keys, annotators | 1, videos); flip: the level reads the second buffer
template <class K, bool FR, bool INV>
__global__ __launch_bounds__(CL_THREADS) void cl_merge_level_kernel(const ClHdr* __restrict__ hdr, K* a0, K* b0, u64* ctr, int w, int flip) {
  const ClHdr h = hdr[blockIdx.z];
  K *ga, *gb; int n;
  if (!cl_seg<K, FR>(h, blockIdx.y, a0, b0, &ga, &gb, &n)) return;
  const long long base = (long long)blockIdx.x * CL_MERGE_BLOCK;
  if (base >= n) return;
  const K* __restrict__ src = flip ? gb : ga;
  K* __restrict__ dst = flip ? ga : gb;
  long long inv = 0;
#pragma unroll
  for (int q = 0; q < CL_MERGE_PER_THREAD; ++q) {
    const long long il = base + q * CL_THREADS + threadIdx.x;
    if (il < n) {
      const int i = (int)il;
      const int s = i & ~(2 * w - 1), mid = min(s + w, n), end = (int)min((long long)s + 2 * (long long)w, (long long)n);
      const K v = src[i];
      int at;
      if (i < mid) {
        const int c = cl_lower<0>(src + mid, end - mid, v);
        inv += c;
        at = i + c;
      } else {
        at = s + (i - mid) + cl_upper<0>(src + s, mid - s, v);
      }
      dst[at] = v;
    }
  }
  if (INV) cl_add_block<CL_THREADS>(ctr + 2 * (h.u_off + blockIdx.y) + 1, inv);
}

namespace {
// sorts every array of the call; returns 1 when the result lies in the second buffer (0: in the first)
template <class K, bool FR, bool INV>
int cl_sort(const ClHdr* hdr, K* a0, K* b0, u64* ctr, int max_n, int users, int n_videos, hipStream_t st) {
  hipLaunchKernelGGL((cl_tile_sort_kernel<K, FR, INV>), dim3((max_n + CL_TILE - 1) / CL_TILE, users, n_videos), dim3(CL_SORT_THREADS), 0, st, hdr, a0, b0, ctr);
  int flip = 0;
  for (long long w = CL_TILE; w < max_n; w <<= 1) {
    hipLaunchKernelGGL((cl_merge_level_kernel<K, FR, INV>), dim3((max_n + CL_MERGE_BLOCK - 1) / CL_MERGE_BLOCK, users, n_videos), dim3(CL_THREADS), 0, st, hdr, a0, b0,
                       ctr, (int)w, flip);
    flip ^= 1;
  }
  return flip;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ prefix sums over the sorted groups
// position j of the sorted groups: its frames << 32 | "its key differs from the one in front" (both sums stay below 2^31)
__device__ __forceinline__ long long cl_scan_item(const u64* __restrict__ s, int j, const sumk_eval_dev_video& v, const ClHdr& h) {
  const u64 key = s[j];
  const long long c = cl_group_frames(v, h, (int)(uint32_t)key);
  return (c << 32) | ((j > 0 && (s[j - 1] >> 32) != (key >> 32)) ? 1 : 0);
}
// exclusive prefix sum over a block of CL_THREADS threads (every thread calls it); *total = the block's sum
__device__ __forceinline__ long long cl_block_scan(long long x, long long* s_w, long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  long long base = 0, tot = 0;
  for (int q = 0; q < CL_THREADS / 64; ++q) { const long long c = s_w[q]; base += q < wave ? c : 0; tot += c; }
  *total = tot;
  return base + incl - x;
}

// grid (scan blocks, videos); apply = 0: the block's sum to gbs; 1: the prefix sums, gbs now holding the sums of the blocks in front
__global__ __launch_bounds__(CL_THREADS) void cl_scan_kernel(ClArgs a, const u64* __restrict__ sorted, int apply) {
  __shared__ long long s_w[CL_THREADS / 64];
  const ClHdr h = a.hdr[blockIdx.y];
  if (h.bad) return;
  const int base = blockIdx.x * CL_SCAN_BLOCK;
  if (base >= h.n_grp) return;
  const sumk_eval_dev_video v = a.vids[blockIdx.y];
  const u64* s = sorted + h.g_off;
  long long item[CL_SCAN_PER_THREAD], sum = 0;
#pragma unroll
  for (int q = 0; q < CL_SCAN_PER_THREAD; ++q) {
    const int j = base + threadIdx.x * CL_SCAN_PER_THREAD + q;
    item[q] = j < h.n_grp ? cl_scan_item(s, j, v, h) : 0;
    sum += item[q];
  }
  long long total;
  long long run = cl_block_scan(sum, s_w, &total);
  if (!apply) { if (threadIdx.x == 0) a.gbs[h.sb_off + blockIdx.x] = total; return; }
  run += a.gbs[h.sb_off + blockIdx.x];
#pragma unroll
  for (int q = 0; q < CL_SCAN_PER_THREAD; ++q) {
    const int j = base + threadIdx.x * CL_SCAN_PER_THREAD + q;
    run += item[q];
    if (j < h.n_grp) { a.gp[h.g_off + j] = (int)(run >> 32); a.gd[h.g_off + j] = (int)(run & 0xffffffffll); }      // inclusive: frames up to j, distinct keys below j's
  }
}
// the sums of a video's scan blocks -> the sums in front of each: grid (videos), SEL_THREADS threads
__global__ __launch_bounds__(SEL_THREADS) void cl_scan_blocks_kernel(ClArgs a) {
  __shared__ long long s_wsum[SEL_WAVES];
  const ClHdr h = a.hdr[blockIdx.x];
  if (h.bad) return;
  const int nsb = (h.n_grp + CL_SCAN_BLOCK - 1) / CL_SCAN_BLOCK;
  long long* bs = a.gbs + h.sb_off;
  long long carry = 0;
  for (int r = 0; r < nsb; r += SEL_THREADS) {
    const int i = r + threadIdx.x;
    const long long x = i < nsb ? bs[i] : 0;
    long long total;
    const long long ex = sel_scan(x, s_wsum, &total);
    if (i < nsb) bs[i] = carry + ex;
    carry += total;
  }
}

// ranks and ties of the groups: grid (group chunks, videos).  Spearman: rank[group]; Kendall: xr[group] and the video's xtie
__global__ __launch_bounds__(CL_THREADS) void cl_group_finish_kernel(ClArgs a, const u64* __restrict__ sorted) {
  const ClHdr h = a.hdr[blockIdx.y];
  if (h.bad || blockIdx.x * CL_THREADS >= h.n_grp) return;
  const int j = blockIdx.x * CL_THREADS + threadIdx.x;
  const u64* s = sorted + h.g_off;
  const int* P = a.gp + h.g_off;
  long long xt = 0;
  if (j < h.n_grp) {
    const u64 key = s[j];
    const int lo = cl_lower<32>(s, h.n_grp, key), hi = cl_upper<32>(s, h.n_grp, key), g = (int)(uint32_t)key;
    const long long p_lo = lo > 0 ? P[lo - 1] : 0, p_hi = P[hi - 1];
    const long long equal = p_hi - p_lo, greater = (long long)h.n_frames - p_hi;
    if (a.kendall) {
      a.xr[h.g_off + g] = a.gd[h.g_off + j];
      if (j == lo) xt = equal * (equal - 1) / 2;
    } else {
      a.rank[h.g_off + g] = (double)greater + 0.5 * ((double)equal + 1.0);      // average of the 1-based positions greater + 1 .. greater + equal
    }
  }
  if (a.kendall) cl_add_block<CL_THREADS>(a.ctr + 2 * a.total_users + blockIdx.y, xt);
}

// ------------------------------------------------------------------------------------------------ Spearman
// grid (chunks, videos): part[(part_off + chunk) * CL_SLOTS + u] = sum over the chunk's frames of (rank - mean)(rank_u - mean_u), slot
// ED_MAX_USERS = the chunk's share of smm, taken over its share of the groups
__global__ __launch_bounds__(CL_THREADS) void cl_spearman_part_kernel(ClArgs a) {
  __shared__ double s_red[CL_THREADS / 64][CL_SLOTS];
  __shared__ double s_um[ED_MAX_USERS];
  const ClHdr h = a.hdr[blockIdx.y];
  const int c = blockIdx.x, tid = threadIdx.x;
  if (h.bad || c >= h.n_chunks) return;
  const sumk_eval_dev_video v = a.vids[blockIdx.y];
  const int n = h.n_frames, nu = h.n_users, nc = h.n_chunks;
  if (tid < nu) s_um[tid] = v.user_mean[tid];
  __syncthreads();
  const double* __restrict__ rank = a.rank + h.g_off;
  const double mean = 0.5 * ((double)n + 1.0);
  double acc[ED_MAX_USERS];
#pragma unroll
  for (int u = 0; u < ED_MAX_USERS; ++u) acc[u] = 0.0;
  const int per = (n + nc - 1) / nc;
  const long long f_end = min((long long)n, (long long)(c + 1) * per);
  for (long long fl = (long long)c * per + tid; fl < f_end; fl += CL_THREADS) {
    const int f = (int)fl;
    const double dm = rank[cl_group_of(v.picks, h.n_int, f)] - mean;
#pragma unroll
    for (int u = 0; u < ED_MAX_USERS; ++u)
      if (u < nu) acc[u] += dm * (v.user_ranks[(long long)u * n + f] - s_um[u]);
  }
  double smm = 0.0;
  const int per_g = (h.n_grp + nc - 1) / nc;
  const long long g_end = min((long long)h.n_grp, (long long)(c + 1) * per_g);
  for (long long gl = (long long)c * per_g + tid; gl < g_end; gl += CL_THREADS) {
    const double dm = rank[gl] - mean;
    smm += (double)cl_group_frames(v, h, (int)gl) * (dm * dm);
  }
  // block reduction in a fixed order: lanes by xor butterflies, then the waves in order
  const int lane = tid & 63, wave = tid >> 6;
  for (int u = 0; u <= nu; ++u) {
    double x = smm;
    if (u < nu) {
      x = 0.0;
#pragma unroll
      for (int q = 0; q < ED_MAX_USERS; ++q) x = q == u ? acc[q] : x;      // (a compile-time-unrollable select keeps acc in registers)
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    if (lane == 0) s_red[wave][u] = x;
  }
  __syncthreads();
  double* out = a.part + (h.part_off + c) * CL_SLOTS;
  for (int u = tid; u <= nu; u += CL_THREADS) out[u < nu ? u : ED_MAX_USERS] = (s_red[0][u] + s_red[1][u]) + (s_red[2][u] + s_red[3][u]);
}

// grid (videos): the chunks' sums in chunk order, then the mean correlation as eval_spearman_final_kernel takes it
__global__ __launch_bounds__(64) void cl_spearman_final_kernel(ClArgs a, double* __restrict__ corr) {
  __shared__ double s_sum[CL_SLOTS];
  const ClHdr h = a.hdr[blockIdx.x];
  if (h.bad) { if (threadIdx.x == 0) corr[blockIdx.x] = nan(""); return; }
  const sumk_eval_dev_video v = a.vids[blockIdx.x];
  const double* p = a.part + h.part_off * CL_SLOTS;
  const int u = threadIdx.x, nu = h.n_users;
  if (u < nu || u == ED_MAX_USERS) {
    double s = 0.0;
    for (int c = 0; c < h.n_chunks; ++c) s += p[(size_t)c * CL_SLOTS + u];
    s_sum[u] = s;
  }
  __syncthreads();
  if (u == 0) {
    if (s_sum[ED_MAX_USERS] != s_sum[ED_MAX_USERS]) { corr[blockIdx.x] = nan(""); return; }
    double c = 0.0;
    for (int q = 0; q < nu; ++q) c += s_sum[q] / sqrt(v.user_ssq[q] * s_sum[ED_MAX_USERS]);
    corr[blockIdx.x] = c / (double)nu;
  }
}

// ------------------------------------------------------------------------------------------------ Kendall
// frame keys of every annotator: grid (frame chunks, videos)
__global__ __launch_bounds__(CL_THREADS) void cl_frame_keys_kernel(ClArgs a) {
  const ClHdr h = a.hdr[blockIdx.y];
  const int f = blockIdx.x * CL_THREADS + threadIdx.x;
  if (h.bad || f >= h.n_frames) return;
  const sumk_eval_dev_video v = a.vids[blockIdx.y];
  const int32_t* __restrict__ y = a.kds[blockIdx.y].y_dense;
  const u64 x = (u64)(uint32_t)a.xr[h.g_off + cl_group_of(v.picks, h.n_int, f)] << CL_Y_BITS;
  for (int u = 0; u < h.n_users; ++u) {
    const long long at = (long long)u * h.n_frames + f;
    a.fa[h.uf_off + at] = x | ((u64)(uint32_t)y[at] & ((1u << CL_Y_BITS) - 1u));
  }
}

// the joint ties and the y parts in (x, y) order: grid (frame chunks, annotators, videos).  keys: the sorted frame keys; ybuf: the other buffer
__global__ __launch_bounds__(CL_THREADS) void cl_kendall_ties_kernel(ClArgs a, const u64* __restrict__ keys, u64* __restrict__ ybuf) {
  const ClHdr h = a.hdr[blockIdx.z];
  const int u = blockIdx.y, n = h.n_frames;
  if (h.bad || u >= h.n_users || blockIdx.x * CL_THREADS >= n) return;
  const long long off = h.uf_off + (long long)u * n;
  const u64* key = keys + off;
  uint32_t* y = reinterpret_cast<uint32_t*>(ybuf + off);
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  long long nt = 0;
  if (i < n) {
    const u64 c = key[i];
    y[i] = (uint32_t)c & ((1u << CL_Y_BITS) - 1u);
    if (i == 0 || key[i - 1] != c) {      // tied pairs, t (t - 1) / 2 per run, counted at the run's first element
      const long long t = cl_upper<0>(key + i, n - i, c);
      nt = t * (t - 1) / 2;
    }
  }
  cl_add_block<CL_THREADS>(a.ctr + 2 * (h.u_off + u), nt);
}

// grid (videos): tau-b per annotator from the integers, then the mean in numpy's order
__global__ __launch_bounds__(64) void cl_kendall_final_kernel(ClArgs a, double* __restrict__ corr, int64_t* __restrict__ counts) {
  __shared__ double s_tau[ED_MAX_USERS];
  const int vi = blockIdx.x, u = threadIdx.x;
  const ClHdr h = a.hdr[vi];
  const sumk_eval_dev_kendall k = a.kds[vi];
  const int nu = h.n_users;
  if (h.bad) {
    if (u == 0) corr[vi] = nan("");
    if (h.bad == 1 && counts != nullptr && nu <= ED_MAX_USERS && u < nu)
      for (int q = 0; q < 4; ++q) counts[4 * (k.counts0 + u) + q] = -1;
    return;
  }
  if (u < nu) {
    const int64_t n = h.n_frames, tot = n * (n - 1) / 2, xtie = (int64_t)a.ctr[2 * a.total_users + vi], ytie = k.ytie[u];
    const int64_t ntie = (int64_t)a.ctr[2 * (h.u_off + u)], dis = (int64_t)a.ctr[2 * (h.u_off + u) + 1];
    const int64_t cmd = tot - xtie - ytie + ntie - 2 * dis;
    s_tau[u] = kendall_tau_b(cmd, tot, xtie, ytie);
    if (counts != nullptr) {
      int64_t* c = counts + 4 * (k.counts0 + u);
      c[0] = cmd; c[1] = xtie; c[2] = ytie; c[3] = ntie;
    }
  }
  __syncthreads();
  if (u == 0) corr[vi] = np_pairwise_leaf(s_tau, nu) / (double)nu;
}

}  // namespace sumk

using namespace sumk;

namespace {
// what the host can see of a call: SUMK_ERR_ARG with the limit in words, nothing launched
int cl_check(const char* who, const void* scores, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_video* videos_host, int n_videos, const void* workspace,
             size_t workspace_bytes, const void* corr, bool kendall, ClLayout* L) {
  SUMK_ARG(scores && videos_dev && videos_host && workspace && corr, "%s: null pointer", who);
  for (int i = 0; i < n_videos; ++i) {
    const sumk_eval_dev_video& h = videos_host[i];
    SUMK_ARG(h.picks != nullptr, "%s: video %d has no picks", who, i);
    SUMK_ARG(h.n_picks >= 1 && h.n_picks <= CL_MAX_PICKS, "%s: video %d has %d picks (1 .. %d supported)", who, i, h.n_picks, CL_MAX_PICKS);
    SUMK_ARG(h.n_frames >= 1 && h.n_frames <= CL_MAX_FRAMES, "%s: video %d has %d frames (1 .. %d supported)", who, i, h.n_frames, CL_MAX_FRAMES);
    SUMK_ARG(h.n_users <= ED_MAX_USERS, "%s: video %d has %d annotators (at most %d supported)", who, i, h.n_users, ED_MAX_USERS);
  }
  SUMK_ARG(cl_layout(videos_host, n_videos, kendall, L), "%s: the descriptors are past a limit", who);
  SUMK_ARG(workspace_bytes >= L->total, "%s: workspace %zu < required %zu", who, workspace_bytes, L->total);
  SUMK_ARG(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  return SUMK_OK;
}

// prologue, group keys, their sort, the prefix sums, ranks and ties of the groups; *sorted = the buffer that holds the sorted groups
void cl_groups(const ClArgs& a, const ClLayout& L, hipStream_t st) {
  const int n = a.n_videos;
  hipLaunchKernelGGL(cl_prologue_kernel, dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL(cl_group_keys_kernel, dim3((L.max_grp + CL_THREADS - 1) / CL_THREADS, n), dim3(CL_THREADS), 0, st, a);
  const u64* sorted = cl_sort<u64, false, false>(a.hdr, a.ga, a.gb, nullptr, L.max_grp, 1, n, st) ? a.gb : a.ga;
  const dim3 scan_grid((L.max_grp + CL_SCAN_BLOCK - 1) / CL_SCAN_BLOCK, n);
  hipLaunchKernelGGL(cl_scan_kernel, scan_grid, dim3(CL_THREADS), 0, st, a, sorted, 0);
  hipLaunchKernelGGL(cl_scan_blocks_kernel, dim3(n), dim3(SEL_THREADS), 0, st, a);
  hipLaunchKernelGGL(cl_scan_kernel, scan_grid, dim3(CL_THREADS), 0, st, a, sorted, 1);
  hipLaunchKernelGGL(cl_group_finish_kernel, dim3((L.max_grp + CL_THREADS - 1) / CL_THREADS, n), dim3(CL_THREADS), 0, st, a, sorted);
}
}  // namespace

extern "C" size_t sumk_eval_device_spearman_long_workspace_bytes(const sumk_eval_dev_video* videos_host, int32_t n_videos) {
  ClLayout L;
  return cl_layout(videos_host, n_videos, false, &L) ? L.total : 0;
}

extern "C" size_t sumk_eval_device_kendall_long_workspace_bytes(const sumk_eval_dev_video* videos_host, int32_t n_videos) {
  ClLayout L;
  return cl_layout(videos_host, n_videos, true, &L) ? L.total : 0;
}

extern "C" int sumk_eval_device_spearman_long(const float* scores_dev, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_video* videos_host,
                                              int32_t n_videos, void* workspace, size_t workspace_bytes, double* corr_dev, void* stream) {
  SUMK_ARG(n_videos >= 0 && n_videos <= 65535, "eval_device_spearman_long: n_videos=%d (at most 65535)", n_videos);
  if (n_videos == 0) return SUMK_OK;
  ClLayout L;
  SUMK_TRY(cl_check("eval_device_spearman_long", scores_dev, videos_dev, videos_host, n_videos, workspace, workspace_bytes, corr_dev, false, &L));
  const ClArgs a = cl_args(L, (char*)workspace, scores_dev, videos_dev, nullptr, n_videos, false);
  hipStream_t st = (hipStream_t)stream;
  cl_groups(a, L, st);
  hipLaunchKernelGGL(cl_spearman_part_kernel, dim3(L.max_chunks, n_videos), dim3(CL_THREADS), 0, st, a);
  hipLaunchKernelGGL(cl_spearman_final_kernel, dim3(n_videos), dim3(64), 0, st, a, corr_dev);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_eval_device_kendall_long(const float* scores_dev, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_video* videos_host,
                                             const sumk_eval_dev_kendall* kendall_dev, int32_t n_videos, void* workspace, size_t workspace_bytes,
                                             double* corr_dev, int64_t* counts_dev, void* stream) {
  SUMK_ARG(n_videos >= 0 && n_videos <= 65535, "eval_device_kendall_long: n_videos=%d (at most 65535)", n_videos);
  if (n_videos == 0) return SUMK_OK;
  ClLayout L;
  SUMK_ARG(kendall_dev != nullptr, "eval_device_kendall_long: null pointer");
  SUMK_TRY(cl_check("eval_device_kendall_long", scores_dev, videos_dev, videos_host, n_videos, workspace, workspace_bytes, corr_dev, true, &L));
  const ClArgs a = cl_args(L, (char*)workspace, scores_dev, videos_dev, kendall_dev, n_videos, true);
  hipStream_t st = (hipStream_t)stream;
  const long long n_ctr = 2 * L.total_users + n_videos;                                     // the integer counters: ntie, dis per annotator; xtie per video
  hipLaunchKernelGGL(cl_zero_kernel, dim3((unsigned)((n_ctr + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0, st, a.ctr, n_ctr);
  cl_groups(a, L, st);
  if (L.max_users > 0) {
    const int n = n_videos, F = L.max_frames, U = L.max_users;
    hipLaunchKernelGGL(cl_frame_keys_kernel, dim3((F + CL_THREADS - 1) / CL_THREADS, n), dim3(CL_THREADS), 0, st, a);
    const bool in_b = cl_sort<u64, true, false>(a.hdr, a.fa, a.fb, nullptr, F, U, n, st) != 0;
    u64* keys = in_b ? a.fb : a.fa;
    u64* ybuf = in_b ? a.fa : a.fb;
    hipLaunchKernelGGL(cl_kendall_ties_kernel, dim3((F + CL_THREADS - 1) / CL_THREADS, U, n), dim3(CL_THREADS), 0, st, a, (const u64*)keys, ybuf);
    cl_sort<uint32_t, true, true>(a.hdr, reinterpret_cast<uint32_t*>(ybuf), (uint32_t*)nullptr, a.ctr, F, U, n, st);
  }
  hipLaunchKernelGGL(cl_kendall_final_kernel, dim3(n_videos), dim3(64), 0, st, a, corr_dev, counts_dev);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
