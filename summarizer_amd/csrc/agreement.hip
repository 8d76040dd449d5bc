// Inter-annotator agreement on the device (include/sumk.h: sumk_rank_rows, sumk_agreement_f, sumk_agreement_corr): how well the
// annotators of a video agree with EACH OTHER under the two metrics every model here is measured by -- the pairwise F-score of their
// key-shot summaries (evaluate_summary, summarizer/utils/eval.py:125-165, with one annotator in the machine's place) and the pairwise
// rank correlation of their frame scores (evaluate_scores, eval.py:49-72).  The specification is tests/agreement_ref.py, bit for bit.
//
//   rank_rows_kernel       one workgroup per (video, annotator) row: kendall_float_key of the row sorted in LDS (kd_merge_sort); an element's
//                          position range [lo, hi) among the sorted keys gives its average rank of -x, (2n - hi - lo + 1) / 2, and the count
//                          of run heads in front of lo its dense rank; sum t (t - 1) / 2 over the runs = the tied pairs.  The centred
//                          rank is (n - hi - lo) / 2: ssq = sum (n - hi - lo)^2 / 4 from an integer sum, exact.
//   agreement_f_kernel     one workgroup per video: a 32-bit word per frame (bit u = annotator u selected it), 64 frames per wave; the
//                          ballots of the word's bits are the annotators' 64-frame masks, popcounts of their ANDs the overlap counts
//                          (the diagonal: the row sums).  F, the leave-one-out mean and maximum through sel_fscores<float>.
//   agreement_gram_kernel  Spearman: one workgroup per (video, annotator a): sum over the frames of (2 r_a - n - 1)(2 r_b - n - 1) for
//                          every b >= a as integers; rho = (sum / 4) / sqrt(ssq_a ssq_b).
//   agreement_pair_kernel  Kendall: one workgroup per (video, pair a < b): key = dense_a << 14 | dense_b, steps 3 to 5 of
//                          eval_kendall_kernel (sort, runs of equal keys, inversions of the y parts); tau[a][b] and tau[b][a] from the
//                          one sort, the tied pairs of either side from sumk_rank_rows.  When the two rows hold few distinct values
//                          (TVSum grades: 5 x 5) the same integers come from their contingency table in LDS instead of the sorts.
//   agreement_final_kernel one workgroup per video: the diagonal (Kendall), corr[a] = the mean over b != a and the video's mean over a,
//                          float64 in numpy's pairwise order.
// Stream order is the only dependency between the launches: no atomics, no cooperative launch, no host synchronisation.
#include "evaldev_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace sumk {

namespace {
constexpr int AG_MAX_USERS = SUMK_SELECT_MAX_USERS;
constexpr int AG_MAX_FRAMES = 1 << 24;       // the limit of sumk_eval_device_select: counts of frames stay exact in float32
constexpr int AG_MAX_VIDEOS = 65535;         // grid.y
constexpr int AG_F_THREADS = 1024;
constexpr int AG_F_WAVES = AG_F_THREADS / 64;
constexpr int AG_GRAM_THREADS = 256;
constexpr size_t AG_BUF_BYTES = (size_t)KD_MAX_FRAMES * sizeof(uint32_t);
constexpr size_t AG_LDS_BYTES = 2 * AG_BUF_BYTES;
static_assert(AG_MAX_USERS == ED_MAX_USERS && AG_MAX_USERS == 32, "one bit per annotator in a 32-bit word");
static_assert(AG_LDS_BYTES <= 160 * 1024 - 2048, "the rank and pair blocks must fit the CU's LDS");
static_assert(KD_MAX_FRAMES <= (1 << KD_Y_BITS) && 2 * KD_Y_BITS <= 32, "key = dense_a << KD_Y_BITS | dense_b");
static_assert(KD_MAX_FRAMES <= 16 * KD_THREADS, "a thread's chunk of the head scan");
constexpr int AG_TABLE_CELLS = KD_THREADS;   // contingency tables up to this many cells (distinct values of a x distinct values of b): one thread per cell

// the element totals of the caller's buffers: a device descriptor is held to them again before anything is written
struct AgTotals { int64_t rank, row, f, sum, c; };

__device__ __forceinline__ bool ag_scores_ok(const sumk_agreement_video& v, const AgTotals& t) {
  return v.n_sc >= 0 && v.n_sc <= AG_MAX_USERS && v.n_frames >= 1 && v.n_frames <= KD_MAX_FRAMES && v.row0 >= 0 && v.row0 + v.n_sc <= t.row &&
         v.rank0 >= 0 && v.rank0 + (int64_t)v.n_sc * v.n_frames <= t.rank;
}
__device__ __forceinline__ bool ag_corr_ok(const sumk_agreement_video& v, const AgTotals& t) {
  return ag_scores_ok(v, t) && v.c0 >= 0 && v.c0 + (int64_t)v.n_sc * v.n_sc <= t.c;
}

// the block's sum of one value per thread (integers: any order); s_red: one entry per wave.  Ends on a barrier-protected read.
template <int NT>
__device__ __forceinline__ long long ag_block_sum(long long x, long long* s_red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = x;
  __syncthreads();
  long long tot = 0;
  for (int w = 0; w < NT / 64; ++w) tot += s_red[w];
  return tot;
}
// the block's maximum of one int per thread; s_red as above
template <int NT>
__device__ __forceinline__ int ag_block_max(int x, long long* s_red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = max(x, __shfl_xor(x, m, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = x;
  __syncthreads();
  int tot = (int)s_red[0];
  for (int w = 1; w < NT / 64; ++w) tot = max(tot, (int)s_red[w]);
  return tot;
}
}  // namespace

struct RankArgs {
  const sumk_agreement_video* vids;
  double* avg; int32_t* dense; int64_t* ties; double* mean; double* ssq;
  AgTotals tot;
};

// grid (largest n_sc of the call, n_videos)
__global__ __launch_bounds__(KD_THREADS) void rank_rows_kernel(RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ag_lds[];
  __shared__ long long s_red[KD_THREADS / 64];
  __shared__ int s_wcnt[KD_THREADS / 64];
  uint32_t* const buf_a = reinterpret_cast<uint32_t*>(ag_lds);
  uint32_t* const buf_b = reinterpret_cast<uint32_t*>(ag_lds + AG_BUF_BYTES);
  const sumk_agreement_video v = a.vids[blockIdx.y];
  const int tid = threadIdx.x, u = blockIdx.x, n = v.n_frames, lane = tid & 63, wave = tid >> 6;
  if (u >= v.n_sc) return;
  if (!ag_scores_ok(v, a.tot) || v.user_scores == nullptr) {
    // a descriptor past a limit: the row's scalars say so where its slot is inside the outputs, nothing else is written
    const int64_t r = v.row0 + u;
    if (tid == 0 && v.row0 >= 0 && r < a.tot.row) { a.ties[r] = -1; a.mean[r] = nan(""); a.ssq[r] = nan(""); }
    return;
  }
  const float* x = v.user_scores + (size_t)u * n;
  for (int i = tid; i < n; i += KD_THREADS) buf_a[i] = kendall_float_key(x[i]);
  __syncthreads();
  long long unused = 0;
  const uint32_t* sorted = kd_merge_sort(buf_a, buf_b, n, unused);
  int* const prefix = reinterpret_cast<int*>(sorted == buf_a ? buf_b : buf_a);       // dense rank of every sorted position
  // ---- run heads: a contiguous chunk of the sorted keys per thread, an exclusive scan of the chunks' head counts over the block
  const int chunk = (n + KD_THREADS - 1) / KD_THREADS, c0 = min(n, tid * chunk), c1 = min(n, c0 + chunk);
  int heads = 0;
  long long ties = 0;
  for (int i = c0; i < c1; ++i) {
    const uint32_t c = sorted[i];
    if (i == 0 || sorted[i - 1] != c) {
      ++heads;
      const long long t = kd_upper(sorted + i, n - i, c);
      ties += t * (t - 1) / 2;
    }
  }
  int incl = heads;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_wcnt[wave] = incl;
  __syncthreads();
  int run = incl - heads;
  for (int q = 0; q < wave; ++q) run += s_wcnt[q];
  for (int i = c0; i < c1; ++i) {
    if (i == 0 || sorted[i - 1] != sorted[i]) ++run;
    prefix[i] = run - 1;
  }
  __syncthreads();
  // ---- ranks of the frames, in frame order
  double* avg = a.avg + v.rank0 + (size_t)u * n;
  int32_t* dense = a.dense + v.rank0 + (size_t)u * n;
  long long sq = 0;
  for (int i = tid; i < n; i += KD_THREADS) {
    const uint32_t k = kendall_float_key(x[i]);
    const int lo = kd_lower(sorted, n, k), hi = kd_upper(sorted, n, k);
    avg[i] = 0.5 * (double)(2 * n - hi - lo + 1);      // rankdata(-x): the n - hi larger values in front, the mean place inside the run
    dense[i] = prefix[lo];
    const long long q = n - hi - lo;                    // twice the centred rank
    sq += q * q;
  }
  ties = ag_block_sum<KD_THREADS>(ties, s_red);
  sq = ag_block_sum<KD_THREADS>(sq, s_red);
  if (tid == 0) {
    const int64_t r = v.row0 + u;
    a.ties[r] = ties;
    a.mean[r] = (double)((long long)n * (n + 1) / 2) / (double)n;
    a.ssq[r] = 0.25 * (double)sq;
  }
}

struct FArgs {
  const sumk_agreement_video* vids;
  float* F; float* fu_avg; float* fu_max; double* f_avg; double* f_max;
  AgTotals tot;
};

// grid (n_videos)
__global__ __launch_bounds__(AG_F_THREADS) void agreement_f_kernel(FArgs a) {
  __shared__ int s_cnt[AG_MAX_USERS][AG_MAX_USERS];
  __shared__ int s_ov[AG_MAX_USERS][AG_MAX_USERS], s_gs[AG_MAX_USERS][AG_MAX_USERS];
  __shared__ float s_f[AG_MAX_USERS][AG_MAX_USERS];
  __shared__ double s_avg[AG_MAX_USERS], s_max[AG_MAX_USERS];
  const int vi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const sumk_agreement_video v = a.vids[vi];
  const int U = v.n_sum, n = v.n_frames;
  if (U == 0) {
    if (tid == 0) { a.f_avg[vi] = nan(""); a.f_max[vi] = nan(""); }
    return;
  }
  if (U < 0 || U > AG_MAX_USERS || n < 1 || n > AG_MAX_FRAMES || v.user_summary == nullptr || v.f0 < 0 || v.f0 + (int64_t)U * U > a.tot.f ||
      v.sum0 < 0 || v.sum0 + U > a.tot.sum) {
    if (tid == 0) { a.f_avg[vi] = nan(""); a.f_max[vi] = nan(""); }
    return;
  }
  s_cnt[tid >> 5][tid & 31] = 0;
  // ---- overlap counts: lane l holds annotator b = l & 31 against the annotators a = 16 (l >> 5) .. + 15
  const int b = lane & 31, a0 = (lane >> 5) * 16;
  int acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0;
  for (int f0 = wave * 64; f0 < n; f0 += AG_F_THREADS) {      // (a bound per wave: every lane reaches the ballots)
    const int f = f0 + lane;
    uint32_t word = 0;
    if (f < n)
      for (int u = 0; u < U; ++u) word |= (v.user_summary[(size_t)u * n + f] > 0.f ? 1u : 0u) << u;
    unsigned long long mine = 0;
#pragma unroll
    for (int u = 0; u < AG_MAX_USERS; ++u) {
      const unsigned long long m = __ballot((word >> u) & 1u);
      mine = b == u ? m : mine;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned long long other = __shfl(mine, a0 + j, 64);
      acc[j] += __popcll(mine & other);
    }
  }
  for (int w = 0; w < AG_F_WAVES; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < 16; ++j) s_cnt[a0 + j][b] += acc[j];
    }
  }
  __syncthreads();
  // ---- annotator r in the machine's place against the others in index order, then against itself (the diagonal)
  if (tid < U) {
    const int r = tid;
    int m = 0;
    for (int k = 0; k < U; ++k)
      if (k != r) { s_ov[r][m] = s_cnt[r][k]; s_gs[r][m] = s_cnt[k][k]; ++m; }
    double fa = nan(""), fm = nan("");
    if (U >= 2) sel_fscores<float>(s_cnt[r][r], s_ov[r], s_gs[r], U - 1, 1e-8f, s_f[r], &fa, &fm);
    float* row = a.F + v.f0 + (size_t)r * U;
    m = 0;
    for (int k = 0; k < U; ++k)
      if (k != r) row[k] = s_f[r][m++];
    float self;
    double d0, d1;
    sel_fscores<float>(s_cnt[r][r], &s_cnt[r][r], &s_cnt[r][r], 1, 1e-8f, &self, &d0, &d1);
    row[r] = self;
    a.fu_avg[v.sum0 + r] = (float)fa; a.fu_max[v.sum0 + r] = (float)fm;
    s_avg[r] = fa; s_max[r] = fm;
  }
  __syncthreads();
  if (tid == 0) {
    a.f_avg[vi] = U >= 2 ? np_pairwise_leaf(s_avg, U) / (double)U : nan("");
    a.f_max[vi] = U >= 2 ? np_pairwise_leaf(s_max, U) / (double)U : nan("");
  }
}

struct CorrArgs {
  const sumk_agreement_video* vids;
  const double* avg; const int32_t* dense; const int64_t* ties; const double* ssq;
  double* Cm; int64_t* counts; double* corr_user; double* corr;
  int metric;
  AgTotals tot;
};

// Spearman; grid (largest n_sc of the call, n_videos)
__global__ __launch_bounds__(AG_GRAM_THREADS) void agreement_gram_kernel(CorrArgs a) {
  __shared__ long long s_red[AG_GRAM_THREADS / 64];
  const sumk_agreement_video v = a.vids[blockIdx.y];
  const int tid = threadIdx.x, ra = blockIdx.x, U = v.n_sc, n = v.n_frames;
  if (ra >= U || !ag_corr_ok(v, a.tot)) return;               // (past a limit: the final kernel writes the video's NaN)
  const double* r = a.avg + v.rank0;
  long long acc[AG_MAX_USERS];
#pragma unroll
  for (int k = 0; k < AG_MAX_USERS; ++k) acc[k] = 0;
  for (int f = tid; f < n; f += AG_GRAM_THREADS) {
    const long long qa = (long long)(2.0 * r[(size_t)ra * n + f]) - (n + 1);
#pragma unroll
    for (int k = 0; k < AG_MAX_USERS; ++k)
      if (k >= ra && k < U) acc[k] += qa * ((long long)(2.0 * r[(size_t)k * n + f]) - (n + 1));
  }
  const double ssq_a = a.ssq[v.row0 + ra];
  double* Cv = a.Cm + v.c0;
  for (int k = ra; k < U; ++k) {
    long long p = 0;
#pragma unroll
    for (int q = 0; q < AG_MAX_USERS; ++q) p = q == k ? acc[q] : p;      // (a compile-time-unrollable select keeps acc in registers)
    p = ag_block_sum<AG_GRAM_THREADS>(p, s_red);
    if (tid == 0) {
      const double rho = (0.25 * (double)p) / sqrt(ssq_a * a.ssq[v.row0 + k]);
      Cv[(size_t)ra * U + k] = rho; Cv[(size_t)k * U + ra] = rho;
    }
  }
}

// Kendall; grid (pairs of the largest n_sc of the call, n_videos)
__global__ __launch_bounds__(KD_THREADS) void agreement_pair_kernel(CorrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ag_lds[];
  __shared__ long long s_red[KD_THREADS / 64];
  uint32_t* const buf_a = reinterpret_cast<uint32_t*>(ag_lds);
  uint32_t* const buf_b = reinterpret_cast<uint32_t*>(ag_lds + AG_BUF_BYTES);
  const sumk_agreement_video v = a.vids[blockIdx.y];
  const int tid = threadIdx.x, U = v.n_sc, n = v.n_frames;
  if (!ag_corr_ok(v, a.tot)) return;                          // (past a limit: the final kernel writes the video's NaN)
  int p = blockIdx.x, ra = 0;
  if (p >= U * (U - 1) / 2) return;
  while (p >= U - 1 - ra) { p -= U - 1 - ra; ++ra; }
  const int rb = ra + 1 + p;
  const int32_t* da = a.dense + v.rank0 + (size_t)ra * n;
  const int32_t* db = a.dense + v.rank0 + (size_t)rb * n;
  const uint32_t ymask = (1u << KD_Y_BITS) - 1u;
  int ga = 0, gb = 0;
  for (int f = tid; f < n; f += KD_THREADS) {
    const int xa = (int)((uint32_t)da[f] & ymask), xb = (int)((uint32_t)db[f] & ymask);
    ga = max(ga, xa); gb = max(gb, xb);
    buf_a[f] = ((uint32_t)xa << KD_Y_BITS) | (uint32_t)xb;
  }
  ga = ag_block_max<KD_THREADS>(ga, s_red) + 1;               // distinct values of either row: dense ranks are 0 .. groups - 1
  gb = ag_block_max<KD_THREADS>(gb, s_red) + 1;               // (the barriers inside also publish the keys)
  long long ntie = 0, dis = 0;
  if (a.metric != SUMK_AGREEMENT_KENDALL_SORT && ga * gb <= AG_TABLE_CELLS) {
    // ---- few distinct values: the pair counts from the ga x gb contingency table.  cp = the cells rounded up to a power of two;
    // thread (slice, cell) counts the frames of its slice that fall into its cell, the slices are summed per cell.
    const int cells = ga * gb;
    int cp = 1, sh = 0;
    while (cp < cells) { cp <<= 1; ++sh; }
    const int slices = KD_THREADS >> sh, len = (n + slices - 1) / slices, cell = tid & (cp - 1), sl = tid >> sh;
    for (int f = tid; f < n; f += KD_THREADS) { const uint32_t k = buf_a[f]; buf_a[f] = (k >> KD_Y_BITS) * (uint32_t)gb + (k & ymask); }
    __syncthreads();
    int cnt = 0;
    for (int f = min(n, sl * len), f1 = min(n, f + len); f < f1; ++f) cnt += buf_a[f] == (uint32_t)cell ? 1 : 0;
    buf_b[tid] = (uint32_t)cnt;                               // [slice][cell]
    __syncthreads();
    uint32_t* const T = buf_b + KD_THREADS;
    if (tid < cp) {
      uint32_t t = 0;
      for (int q = 0; q < slices; ++q) t += buf_b[q * cp + tid];
      T[tid] = t;
    }
    __syncthreads();
    if (tid < cells) {
      const int i = tid / gb, j = tid - i * gb;
      const long long t = T[tid];
      long long below = 0;                                    // frames with a larger value in a and a smaller one in b: discordant with this cell's
      for (int i2 = i + 1; i2 < ga; ++i2)
        for (int j2 = 0; j2 < j; ++j2) below += T[i2 * gb + j2];
      ntie = t * (t - 1) / 2;
      dis = t * below;
    }
  } else {
    long long unused = 0;
    uint32_t* key = kd_merge_sort(buf_a, buf_b, n, unused);
    uint32_t* other = key == buf_a ? buf_b : buf_a;
    for (int i = tid; i < n; i += KD_THREADS) {
      const uint32_t c = key[i];
      if (i == 0 || key[i - 1] != c) {
        const long long t = kd_upper(key + i, n - i, c);
        ntie += t * (t - 1) / 2;
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += KD_THREADS) key[i] &= ymask;
    __syncthreads();
    kd_merge_sort(key, other, n, dis);
  }
  ntie = ag_block_sum<KD_THREADS>(ntie, s_red);
  dis = ag_block_sum<KD_THREADS>(dis, s_red);
  if (tid == 0) {
    const int64_t tot = (int64_t)n * (n - 1) / 2, xt = a.ties[v.row0 + ra], yt = a.ties[v.row0 + rb];
    const int64_t cmd = tot - xt - yt + ntie - 2 * dis;
    double* Cv = a.Cm + v.c0;
    Cv[(size_t)ra * U + rb] = kendall_tau_b(cmd, tot, xt, yt);
    Cv[(size_t)rb * U + ra] = kendall_tau_b(cmd, tot, yt, xt);
    if (a.counts != nullptr) {
      int64_t* c = a.counts + 4 * (v.c0 + (int64_t)ra * U + rb);
      c[0] = cmd; c[1] = xt; c[2] = yt; c[3] = ntie;
      c = a.counts + 4 * (v.c0 + (int64_t)rb * U + ra);
      c[0] = cmd; c[1] = yt; c[2] = xt; c[3] = ntie;
    }
  }
}

// grid (n_videos), one wave
__global__ __launch_bounds__(64) void agreement_final_kernel(CorrArgs a) {
  __shared__ double s_row[AG_MAX_USERS][AG_MAX_USERS];
  __shared__ double s_corr[AG_MAX_USERS];
  const int vi = blockIdx.x, tid = threadIdx.x;
  const sumk_agreement_video v = a.vids[vi];
  const int U = v.n_sc, n = v.n_frames;
  if (U == 0 || !ag_corr_ok(v, a.tot)) {
    if (tid == 0) a.corr[vi] = nan("");
    return;
  }
  double* Cv = a.Cm + v.c0;
  if (tid < U) {
    const int r = tid;
    if (a.metric != SUMK_AGREEMENT_SPEARMAN) {                // a row against itself: every pair tied on both sides or concordant
      const int64_t tot = (int64_t)n * (n - 1) / 2, t = a.ties[v.row0 + r];
      Cv[(size_t)r * U + r] = kendall_tau_b(tot - t, tot, t, t);
      if (a.counts != nullptr) {
        int64_t* c = a.counts + 4 * (v.c0 + (int64_t)r * U + r);
        c[0] = tot - t; c[1] = t; c[2] = t; c[3] = t;
      }
    }
    int m = 0;
    for (int k = 0; k < U; ++k)
      if (k != r) s_row[r][m++] = Cv[(size_t)r * U + k];
    const double c = U >= 2 ? np_pairwise_leaf(s_row[r], U - 1) / (double)(U - 1) : nan("");
    a.corr_user[v.row0 + r] = c;
    s_corr[r] = c;
  }
  __syncthreads();
  if (tid == 0) a.corr[vi] = U >= 2 ? np_pairwise_leaf(s_corr, U) / (double)U : nan("");
}

namespace {
// what the three entries check on the host copy; *max_sc: the largest n_sc of the call
int ag_check(const char* what, const sumk_agreement_video* h_, int n_videos, bool scores, const AgTotals& t, int* max_sc) {
  SUMK_ARG(n_videos <= AG_MAX_VIDEOS, "%s: %d videos (at most %d per call)", what, n_videos, AG_MAX_VIDEOS);
  int ms = 0;
  for (int i = 0; i < n_videos; ++i) {
    const sumk_agreement_video& h = h_[i];
    SUMK_ARG(h.reserved == 0, "%s: video %d: the reserved field must be 0", what, i);
    SUMK_ARG(h.n_frames >= 1 && h.n_frames <= AG_MAX_FRAMES, "%s: video %d has %d frames (1 .. %d supported)", what, i, h.n_frames, AG_MAX_FRAMES);
    if (scores) {
      SUMK_ARG(h.n_sc >= 0 && h.n_sc <= AG_MAX_USERS, "%s: video %d has %d score rows (at most %d annotators supported)", what, i, h.n_sc, AG_MAX_USERS);
      if (h.n_sc == 0) continue;
      SUMK_ARG(h.user_scores, "%s: video %d: null user_scores", what, i);
      SUMK_ARG(h.n_frames <= KD_MAX_FRAMES, "%s: video %d has %d frames (ranks and correlations: at most %d)", what, i, h.n_frames, KD_MAX_FRAMES);
      SUMK_ARG(h.rank0 >= 0 && h.rank0 + (int64_t)h.n_sc * h.n_frames <= t.rank, "%s: video %d: ranks [%lld, +%d x %d) outside the %lld entries given", what,
               i, (long long)h.rank0, h.n_sc, h.n_frames, (long long)t.rank);
      SUMK_ARG(h.row0 >= 0 && h.row0 + h.n_sc <= t.row, "%s: video %d: rows [%lld, +%d) outside the %lld entries given", what, i, (long long)h.row0,
               h.n_sc, (long long)t.row);
      ms = h.n_sc > ms ? h.n_sc : ms;
    } else {
      SUMK_ARG(h.n_sum >= 0 && h.n_sum <= AG_MAX_USERS, "%s: video %d has %d summaries (at most %d annotators supported)", what, i, h.n_sum, AG_MAX_USERS);
      if (h.n_sum == 0) continue;
      SUMK_ARG(h.user_summary, "%s: video %d: null user_summary", what, i);
      SUMK_ARG(h.f0 >= 0 && h.f0 + (int64_t)h.n_sum * h.n_sum <= t.f, "%s: video %d: F [%lld, +%d x %d) outside the %lld entries given", what, i,
               (long long)h.f0, h.n_sum, h.n_sum, (long long)t.f);
      SUMK_ARG(h.sum0 >= 0 && h.sum0 + h.n_sum <= t.sum, "%s: video %d: annotators [%lld, +%d) outside the %lld entries given", what, i, (long long)h.sum0,
               h.n_sum, (long long)t.sum);
    }
  }
  *max_sc = ms;
  return SUMK_OK;
}
}  // namespace

}  // namespace sumk

using namespace sumk;

extern "C" int sumk_rank_rows(const sumk_agreement_video* videos_dev, const sumk_agreement_video* videos_host, int32_t n_videos,
                              double* avg_ranks_dev, int32_t* dense_ranks_dev, int64_t rank_total, int64_t* ties_dev, double* mean_dev,
                              double* ssq_dev, int64_t row_total, void* stream) {
  SUMK_ARG(n_videos >= 0, "rank_rows: n_videos=%d", n_videos);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(videos_dev && videos_host && avg_ranks_dev && dense_ranks_dev && ties_dev && mean_dev && ssq_dev, "rank_rows: null pointer");
  SUMK_ARG(rank_total >= 0 && row_total >= 0, "rank_rows: negative output size");
  AgTotals t{rank_total, row_total, 0, 0, 0};
  int max_sc = 0;
  SUMK_TRY(ag_check("rank_rows", videos_host, n_videos, true, t, &max_sc));
  if (max_sc == 0) return SUMK_OK;
  RankArgs a{videos_dev, avg_ranks_dev, dense_ranks_dev, ties_dev, mean_dev, ssq_dev, t};
  SUMK_TRY(lds_opt_in<rank_rows_kernel>((int)AG_LDS_BYTES));
  hipLaunchKernelGGL(rank_rows_kernel, dim3(max_sc, n_videos), dim3(KD_THREADS), AG_LDS_BYTES, (hipStream_t)stream, a);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_agreement_f(const sumk_agreement_video* videos_dev, const sumk_agreement_video* videos_host, int32_t n_videos, float* F_dev,
                                int64_t f_total, float* f_avg_user_dev, float* f_max_user_dev, int64_t sum_total, double* f_avg_dev,
                                double* f_max_dev, void* stream) {
  SUMK_ARG(n_videos >= 0, "agreement_f: n_videos=%d", n_videos);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(videos_dev && videos_host && F_dev && f_avg_user_dev && f_max_user_dev && f_avg_dev && f_max_dev, "agreement_f: null pointer");
  SUMK_ARG(f_total >= 0 && sum_total >= 0, "agreement_f: negative output size");
  AgTotals t{0, 0, f_total, sum_total, 0};
  int unused = 0;
  SUMK_TRY(ag_check("agreement_f", videos_host, n_videos, false, t, &unused));
  FArgs a{videos_dev, F_dev, f_avg_user_dev, f_max_user_dev, f_avg_dev, f_max_dev, t};
  hipLaunchKernelGGL(agreement_f_kernel, dim3(n_videos), dim3(AG_F_THREADS), 0, (hipStream_t)stream, a);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_agreement_corr(const sumk_agreement_video* videos_dev, const sumk_agreement_video* videos_host, int32_t n_videos, int32_t metric,
                                   const double* avg_ranks_dev, const int32_t* dense_ranks_dev, int64_t rank_total, const int64_t* ties_dev,
                                   const double* ssq_dev, int64_t row_total, double* C_dev, int64_t c_total, int64_t* counts_dev,
                                   double* corr_user_dev, double* corr_dev, void* stream) {
  SUMK_ARG(n_videos >= 0, "agreement_corr: n_videos=%d", n_videos);
  SUMK_ARG(metric == SUMK_AGREEMENT_SPEARMAN || metric == SUMK_AGREEMENT_KENDALL || metric == SUMK_AGREEMENT_KENDALL_SORT,
           "agreement_corr: metric %d (0 = Spearman, 1 = Kendall, 2 = Kendall through the sort alone)", metric);
  if (n_videos == 0) return SUMK_OK;
  SUMK_ARG(videos_dev && videos_host && avg_ranks_dev && dense_ranks_dev && ties_dev && ssq_dev && C_dev && corr_user_dev && corr_dev,
           "agreement_corr: null pointer");
  SUMK_ARG(rank_total >= 0 && row_total >= 0 && c_total >= 0, "agreement_corr: negative buffer size");
  AgTotals t{rank_total, row_total, 0, 0, c_total};
  int max_sc = 0;
  SUMK_TRY(ag_check("agreement_corr", videos_host, n_videos, true, t, &max_sc));
  for (int i = 0; i < n_videos; ++i) {
    const sumk_agreement_video& h = videos_host[i];
    SUMK_ARG(h.n_sc == 0 || (h.c0 >= 0 && h.c0 + (int64_t)h.n_sc * h.n_sc <= c_total), "agreement_corr: video %d: C [%lld, +%d x %d) outside the %lld entries given",
             i, (long long)h.c0, h.n_sc, h.n_sc, (long long)c_total);
  }
  CorrArgs a{videos_dev, avg_ranks_dev, dense_ranks_dev, ties_dev, ssq_dev, C_dev, counts_dev, corr_user_dev, corr_dev, metric, t};
  if (metric == SUMK_AGREEMENT_SPEARMAN) {
    if (max_sc > 0) hipLaunchKernelGGL(agreement_gram_kernel, dim3(max_sc, n_videos), dim3(AG_GRAM_THREADS), 0, (hipStream_t)stream, a);
  } else if (max_sc > 1) {
    SUMK_TRY(lds_opt_in<agreement_pair_kernel>((int)AG_LDS_BYTES));
    hipLaunchKernelGGL(agreement_pair_kernel, dim3(max_sc * (max_sc - 1) / 2, n_videos), dim3(KD_THREADS), AG_LDS_BYTES, (hipStream_t)stream, a);
  }
  SUMK_HIP(hipGetLastError());
  hipLaunchKernelGGL(agreement_final_kernel, dim3(n_videos), dim3(64), 0, (hipStream_t)stream, a);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
