// Banded, chip-wide kernel temporal segmentation: sumk_kts (kts.hip) for videos the dense path cannot hold or would run on one CU.
// Same definition, same outputs and -- inside the band -- the same arithmetic in the same order, so for every input both paths accept
// n_cps, cps and the BITS of scores are those of sumk_kts (tests/test_gpu_kts_banded.py).  Two things differ.
//
// 1. Band storage.  The DP only reads J[t][l - 1] with l - t <= lmax, so with B = min(lmax, n) a video keeps J[t][t .. t + B - 1] only:
//      J band   double [n][B]     row t, entry c = column t + c  (c = 0 is the diagonal); entries with t + c >= n are never written or used
//      Gram     float  [n][ldg]   64-row strips; strip r = rows 64 r .. 64 r + 63 is ONE problem of the lean NT launch (gemm_lean.hip, the same
//                                 kernel and K loop as the dense path), a rectangle of min(n - 64 r, B + 63) columns that starts at its own
//                                 diagonal column 64 r: entry (s, j) sits at s ldg + (j - 64 (s / 64)), ldg = min(n, B + 63) rounded up to 4
//    The workspace is O(n B) instead of O(n^2); every offset is 64-bit.  The Gram strips share their bytes with p and the I rows of the
//    DP, which are first written when the strips are dead.
//      column pass  W[s][j] = K[j][j] + sum_{s <= s' < j} 2 K[s'][j], s descending from the diagonal and stopping at j - s = B - 1.  One wave per
//                   64 columns walks s down TOGETHER (lane j joins at s = j and leaves after s = j - B + 1): the lanes of one step then read
//                   one Gram row and write one band row, both contiguous -- the per-lane order of additions is the dense one.
//      row pass     the two inclusive scans from t = i in chunks of 64 with the carry (kts_row_scan, kts_common.h), over the min(B, n - i) entries of row i.
// 2. A DP row is a launch.  Row k depends on the whole of row k - 1, and the only chip-wide ordering that needs no barrier, no cooperative
//    launch, no spin-wait and no atomics is the stream: k launches, each over all end points l of all videos.  A block owns 64 consecutive end
//    points (lane = l: the reads of J[t][l - 1 - t] at a fixed t are 64 consecutive doubles) and its 16 waves cut the window
//    max(k lmin, l - lmax) <= t < l into 16 ascending pieces; the partial minima meet in LDS under an explicit (value, index) compare, so the
//    smallest t still wins a tie.  A row streams every band entry it needs exactly once: at most n B doubles (n^2 / 2 when B = n), spread
//    over ceil(n / 64) blocks instead of one.  Rows with (k + 1) lmin > n are not launched (the host knows n).  p is int32 for every n.
//    The closing launch (one block per video) runs the tail both paths share (kts_tail, kts_common.h): penalty, arg-min over k, backtrack,
//    score row.
// Nothing waits on the host: the call enqueues 6 + (number of DP rows) launches.
#include "kts_common.h"

namespace sumk {

namespace {
constexpr int KB_MAX_N = 1048576;
constexpr int KB_DP_THREADS = 1024, KB_DP_WAVES = KB_DP_THREADS / 64;
constexpr int KB_J_PAD = 64;                                // doubles behind the last band: lanes outside their window read (and drop) up to 63 past a row

struct BSeq {
  int64_t goff;    // fp32 Gram strips: element offset
  int64_t joff;    // float64 band: element offset (sum of n B)
  int64_t poff;    // p: element offset (int32)
  int64_t ioff;    // the two I rows: element offset (sum of 2 (n + 1))
  int32_t row0, n, ldg, m, B, pad_[3];
};

struct KbWs { size_t gram, J, diag, p, irows, sc, seq, prob, total; int32_t n_max, tiles, nprob; };

int kb_carve(int D, int n_seq, const int32_t* off, int max_ncp, int lmax, KbWs* w) {
  SUMK_ARG(D > 0 && D % 4 == 0, "kts_banded: D=%d must be a positive multiple of 4", D);
  SUMK_ARG(n_seq > 0 && n_seq <= 65535 && off && off[0] == 0, "kts_banded: empty batch (or more than 65535 videos)");
  SUMK_ARG(lmax >= 1, "kts_banded: need 1 <= lmin <= lmax, got lmax=%d", lmax);
  int n_max = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int64_t n = (int64_t)off[s + 1] - off[s];
    SUMK_ARG(n >= 1 && n <= KB_MAX_N, "kts_banded: video %d has %lld steps (1 .. %d supported)", s, (long long)n, KB_MAX_N);
    n_max = n > n_max ? (int)n : n_max;
  }
  SUMK_ARG(max_ncp >= 0 && max_ncp <= n_max - 1, "kts_banded: max_ncp=%d outside 0 .. %d (longest video - 1)", max_ncp, n_max - 1);
  size_t g = 0, j = 0, pe = 0, ir = 0; int64_t tiles = 0, nprob = 0;
  for (int s = 0; s < n_seq; ++s) {
    const KtsBandSizes z = kts_band_sizes(off[s + 1] - off[s], max_ncp, lmax);
    g += z.gram; j += z.J; pe += z.p; ir += z.irows;
    tiles += z.tiles; nprob += z.probs;
  }
  SUMK_ARG(tiles < ((int64_t)1 << 31), "kts_banded: %lld Gram tiles do not fit one launch: use a smaller lmax", (long long)tiles);
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  // the fp32 Gram is dead once the column pass has run, p and the I rows are first written after the row pass: they share one region
  const size_t gb = align_up(g * 4, 256), pb = align_up(pe * 4, 256), ib = align_up(ir * 8, 256);
  w->gram = take(gb > pb + ib ? gb : pb + ib);
  w->p = w->gram; w->irows = w->gram + pb;
  w->J = take((j + KB_J_PAD) * 8);
  w->diag = take((size_t)off[n_seq] * 8);
  w->sc = take((size_t)n_seq * ((size_t)max_ncp + 1) * 8);
  w->seq = take((size_t)n_seq * sizeof(BSeq));
  w->prob = take((size_t)nprob * sizeof(GemmProb));
  w->total = p; w->n_max = n_max; w->tiles = (int32_t)tiles; w->nprob = (int32_t)nprob;
  return SUMK_OK;
}
}  // namespace

// One thread per video: its offsets (the sums of kts_band_sizes over the videos before it, as kb_carve adds them) and one GEMM problem
// per 64-row strip of its Gram band.
__global__ void kts_banded_setup_kernel(const int32_t* off, int n_seq, int D, int max_ncp, int lmax, BSeq* seq, GemmProb* prob) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  int64_t goff = 0, joff = 0, poff = 0, ioff = 0; int ts = 0, pi = 0;
  for (int q = 0; q < s; ++q) {
    const KtsBandSizes z = kts_band_sizes(off[q + 1] - off[q], max_ncp, lmax);
    goff += z.gram; joff += z.J; poff += z.p; ioff += z.irows;
    ts += z.tiles; pi += z.probs;
  }
  const int row0 = off[s], n = off[s + 1] - row0;
  const KtsBandSizes z = kts_band_sizes(n, max_ncp, lmax);
  BSeq k; k.goff = goff; k.joff = joff; k.poff = poff; k.ioff = ioff;
  k.row0 = row0; k.n = n; k.ldg = z.ldg; k.m = z.m; k.B = z.B; k.pad_[0] = k.pad_[1] = k.pad_[2] = 0;
  seq[s] = k;
  for (int r = 0; r < z.probs; ++r)
    ts += kts_strip_prob(prob + pi + r, row0, n, r, D, kts_band_strip_n(n, z.B, r), goff + (int64_t)64 * r * z.ldg, z.ldg, ts);
}

// Column pass.  One wave per 64 columns; the wave walks s down from its last column, lane j takes part while j - B < s <= j.
__global__ __launch_bounds__(256) void kts_banded_col_kernel(const float* __restrict__ G, const BSeq* __restrict__ seq, double* __restrict__ W,
                                                             double* __restrict__ diag) {
  const BSeq si = seq[blockIdx.y];
  const int n = si.n, B = si.B;
  const int j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (j0 >= n) return;
  const int j = j0 + (threadIdx.x & 63);
  const bool live = j < n;
  const float* g = G + si.goff;
  double* w = W + si.joff;
  const int s_hi = j0 + 63 < n - 1 ? j0 + 63 : n - 1, s_lo = j0 - B + 1 > 0 ? j0 - B + 1 : 0;
  double acc = 0.0;
#pragma unroll 4
  for (int s = s_hi; s >= s_lo; --s) {
    if (live && s <= j && j - s < B) {
      const double v = (double)g[(int64_t)s * si.ldg + (j - (s & ~63))];
      if (s == j) { acc = v; diag[si.row0 + j] = v; }
      else acc += 2.0 * v;
      w[(int64_t)s * B + (j - s)] = acc;
    }
  }
}

// Row pass: one wave per row i; kts_row_scan over the min(B, n - i) band entries of the row, J over W.
__global__ __launch_bounds__(256) void kts_banded_row_kernel(const BSeq* __restrict__ seq, double* __restrict__ W, const double* __restrict__ diag) {
  const BSeq si = seq[blockIdx.y];
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), n = si.n;
  if (i >= n) return;
  kts_row_scan(W + si.joff + (int64_t)i * si.B, diag + si.row0 + i, n - i < si.B ? n - i : si.B, threadIdx.x & 63);
}

struct KbArgs {
  const BSeq* seq; const double* J; int32_t* p; double* irows; double* sc;
  int32_t max_ncp, lmin, lmax, k; double vmax;
  int32_t* n_cps; int32_t* cps; double* scores;
};

// DP row 0: I[0][l] = J[0][l - 1] for lmin <= l < lmax (EXCLUSIVE: the kept quirk), KTS_BIG elsewhere; l - 1 <= B - 1 there.
__global__ __launch_bounds__(256) void kts_banded_row0_kernel(KbArgs a) {
  const BSeq si = a.seq[blockIdx.y];
  const int l = blockIdx.x * 256 + threadIdx.x, n = si.n;
  if (l > n) return;
  const double v = (l >= a.lmin && l < a.lmax) ? a.J[si.joff + (l - 1)] : KTS_BIG;
  a.irows[si.ioff + l] = v;
  if (l == n) a.sc[(int64_t)blockIdx.y * (a.max_ncp + 1)] = v;
}

// DP row k >= 1.  Block = 64 end points l (lane = l), 16 waves = 16 ascending pieces of the window; see the head of the file.
__global__ __launch_bounds__(KB_DP_THREADS) void kts_banded_dp_kernel(KbArgs a) {
  __shared__ double red_v[KB_DP_WAVES][64];
  __shared__ int red_t[KB_DP_WAVES][64];
  const BSeq si = a.seq[blockIdx.y];
  const int n = si.n, k = a.k;
  const int64_t lstart = (int64_t)(k + 1) * a.lmin;
  if (k > si.m || lstart > n) return;                         // this video has no row k (uniform over the block)
  const int64_t l0w = lstart + (int64_t)blockIdx.x * 64;
  if (l0w > n) return;
  const int l0 = (int)l0w, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = l0 + lane, tlo = k * a.lmin;                  // (k lmin < lstart <= n)
  const bool live = l <= n;
  const int t0 = l - a.lmax > tlo ? l - a.lmax : tlo;         // this end point's window: t0 <= t < l
  const int l_last = l0 + 63 < n ? l0 + 63 : n;
  const int tA = l0 - a.lmax > tlo ? l0 - a.lmax : tlo, tB = l_last;      // the block's: tA <= t < tB
  const int piece = (tB - tA + KB_DP_WAVES - 1) / KB_DP_WAVES;
  const int ta = tA + wave * piece, tb = ta + piece < tB ? ta + piece : tB;
  const double* __restrict__ prev = a.irows + si.ioff + (int64_t)((k - 1) & 1) * (n + 1);
  const double* __restrict__ J = a.J + si.joff;
  const int64_t B = si.B;
  double best = INFINITY; int arg = 0x7fffffff;
  // Band entry of row t for this lane: J[t B + (l - 1 - t)] = Jl[t (B - 1)].  Inside the lane's window 0 <= l - 1 - t <= B - 1; outside it (the
  // corners of the block's parallelogram, lanes past n) the address still lies in the band or in the KB_J_PAD doubles behind it and the value
  // is dropped.  Eight independent loads are issued before the first compare: the loop lives on memory-level parallelism.
  const double* __restrict__ Jl = J + (l - 1);
  const int64_t Bm1 = B - 1;
  int t = ta;
  for (; t + 8 <= tb; t += 8) {
    double jv[8], pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { jv[u] = Jl[(int64_t)(t + u) * Bm1]; pv[u] = prev[t + u]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double v = pv[u] + jv[u];
      if (live && t + u >= t0 && t + u < l && v < best) { best = v; arg = t + u; }      // ascending t, strict compare: the smallest t of the piece
    }
  }
  for (; t < tb; ++t) {
    const double v = prev[t] + Jl[(int64_t)t * Bm1];
    if (live && t >= t0 && t < l && v < best) { best = v; arg = t; }
  }
  red_v[wave][lane] = best; red_t[wave][lane] = arg;
  __syncthreads();
  if (wave == 0 && live) {
    for (int q = 1; q < KB_DP_WAVES; ++q) {
      const double v = red_v[q][lane]; const int t = red_t[q][lane];
      if (v < best || (v == best && t < arg)) { best = v; arg = t; }
    }
    if (arg == 0x7fffffff) arg = t0;                          // nothing below +inf: the sequential loop's start value
    a.irows[si.ioff + (int64_t)(k & 1) * (n + 1) + l] = best;
    a.p[si.poff + (int64_t)(k - 1) * (n + 1) + l] = arg;
    if (l == n) a.sc[(int64_t)blockIdx.y * (a.max_ncp + 1) + k] = best;
  }
}

// Closing launch, one block per video: the rows that were not run read KTS_BIG, then kts_tail (penalty + arg-min over k with the
// smallest k at a tie, backtrack, score row).
__global__ __launch_bounds__(KTS_TAIL_THREADS) void kts_banded_tail_kernel(KbArgs a) {
  __shared__ double red[KTS_TAIL_THREADS / 64];
  __shared__ int redk[KTS_TAIL_THREADS / 64];
  const int v = blockIdx.x, tid = threadIdx.x;
  const BSeq si = a.seq[v];
  const int n = si.n, m = si.m;
  const int32_t* p = a.p + si.poff;
  double* sc = a.sc + (int64_t)v * (a.max_ncp + 1);
  const int64_t kfeas = (int64_t)n / a.lmin;                  // rows 1 .. kfeas - 1 have (k + 1) lmin <= n
  const int krun = kfeas - 1 < m ? (int)(kfeas - 1 > 0 ? kfeas - 1 : 0) : m;
  for (int q = krun + 1 + tid; q <= m; q += KTS_TAIL_THREADS) sc[q] = KTS_BIG;
  __syncthreads();
  const KtsTail t = {a.max_ncp, a.lmin, 0, a.vmax, a.n_cps, a.cps, a.scores};
  kts_tail(t, v, n, m, sc, red, redk, [&](int64_t idx) { return p[idx]; });
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_kts_banded_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t max_ncp, int32_t lmax) {
  KbWs w;
  if (kb_carve(D, n_seq, seq_off_host, max_ncp, lmax, &w) != SUMK_OK) return 0;
  return w.total;
}

extern "C" int sumk_kts_banded(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                               int32_t max_ncp, int32_t lmin, int32_t lmax, double vmax, int32_t* n_cps, int32_t* cps, double* scores,
                               void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_TRY(kts_check_args("kts_banded", x, seq_off_dev, n_cps, cps, workspace, max_ncp, lmin, lmax, vmax));
  KbWs L;
  SUMK_TRY(kb_carve(D, n_seq, seq_off_host, max_ncp, lmax, &L));
  SUMK_ARG(workspace_bytes >= L.total, "kts_banded: workspace %zu < required %zu", workspace_bytes, L.total);
  char* ws = (char*)workspace;
  float* G = (float*)(ws + L.gram);
  double* W = (double*)(ws + L.J);
  double* diag = (double*)(ws + L.diag);
  BSeq* seq = (BSeq*)(ws + L.seq);
  GemmProb* prob = (GemmProb*)(ws + L.prob);
  hipLaunchKernelGGL(kts_banded_setup_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, seq_off_dev, n_seq, D, max_ncp, lmax, seq, prob);
  GemmLaunch g;
  g.A = x; g.B[0] = x; g.C = G; g.probs = prob; g.nprob = L.nprob; g.small_tile = 1; g.total_tiles = L.tiles;
  SUMK_TRY(launch_gemm(GEMM_NT, EPI_NONE, g, stream));
  hipLaunchKernelGGL(kts_banded_col_kernel, dim3((L.n_max + 255) / 256, n_seq), dim3(256), 0, stream, G, seq, W, diag);
  hipLaunchKernelGGL(kts_banded_row_kernel, dim3((L.n_max + 3) / 4, n_seq), dim3(256), 0, stream, seq, W, diag);
  KbArgs a;
  a.seq = seq; a.J = W; a.p = (int32_t*)(ws + L.p); a.irows = (double*)(ws + L.irows); a.sc = (double*)(ws + L.sc);
  a.max_ncp = max_ncp; a.lmin = lmin; a.lmax = lmax; a.k = 0; a.vmax = vmax;
  a.n_cps = n_cps; a.cps = cps; a.scores = scores;
  hipLaunchKernelGGL(kts_banded_row0_kernel, dim3(L.n_max / 256 + 1, n_seq), dim3(256), 0, stream, a);
  // rows the longest video can have: k <= m and (k + 1) lmin <= n; a shorter video's blocks leave at once
  const int64_t kfeas = (int64_t)L.n_max / lmin - 1;
  const int k_last = kfeas < max_ncp ? (int)kfeas : max_ncp;
  for (int k = 1; k <= k_last; ++k) {
    a.k = k;
    const int64_t lstart = (int64_t)(k + 1) * lmin;
    hipLaunchKernelGGL(kts_banded_dp_kernel, dim3((unsigned)((L.n_max - lstart) / 64 + 1), n_seq), dim3(KB_DP_THREADS), 0, stream, a);
  }
  hipLaunchKernelGGL(kts_banded_tail_kernel, dim3(n_seq), dim3(KTS_TAIL_THREADS), 0, stream, a);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
