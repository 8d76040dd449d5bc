// Kernel temporal segmentation (KTS, Potapov et al. 2014) of a packed batch: change points from features, on the device.
// No reference counterpart: the reference reads `change_points` / `n_frame_per_seg` that somebody prepared offline with KTS
// (summarizer/datasets/README.md); this file is that preparation step, so a scorer's output can become key shots for any video.
//
//   K      = X X^T per video                          exact fp32, the per-video lean NT launch (gemm_lean.hip), upper tile triangle only
//   J[i,j] = sum_{t=i..j} K[t,t] - (1 / (j - i + 1)) sum_{s,t=i..j} K[s,t]      scatter of the segment i..j, float64
//   I[0,l] = J[0,l-1] (lmin <= l < lmax), I[k,l] = min_{t0 <= t < l} I[k-1,t] + J[t,l-1],  p[k,l] = the SMALLEST minimising t
//   cost[k] = I[k,n] / n + (vmax k / (2 n)) (ln(n / k) + 1),  m_best = the SMALLEST minimising k;  backtrack through p from row m_best
//
// Everything behind the Gram matrix is float64: J is a difference of sums of up to n^2 Gram entries, and in fp32 that cancellation
// would decide change points.  J is built in ONE (n x n) float64 array per video, in place, in two passes:
//   column pass  W[s][j] = K[j][j] + sum_{s <= s' < j} (K[s'][j] + K[j][s'])   (one thread per column j, s descending) -- the increment
//                S(s, j) - S(s, j - 1) of the block sum S(i, j) = sum_{s,t=i..j} K[s,t];
//   row pass     S(i, j) = sum_{t=i..j} W[i][t] and the diagonal sum as two wave scans along row i, J[i][j] written over W[i][j].
// That is the 2-D prefix sum of the definition with the two cumulative sums started at the segment's own corner instead of at (0, 0):
// every J adds only the entries of its own block (no P[j,j] + P[i,i] - P[j,i] - P[i,j] cancellation of four n^2-sized sums), needs no
// second (n + 1)^2 array, and leaves J laid out [t][l - 1]: for a fixed t consecutive l are consecutive doubles, which is how the DP
// reads it (lane = l).  The features path reads only s <= j of the fp32 Gram (K is symmetric there: K[s][j] + K[j][s] = 2 K[s][j], exact),
// so the GEMM writes only the tiles on and above the diagonal.
//
// DP: one workgroup per video, threads strided over the end point l, two rows of I double-buffered in LDS when they fit (n <= 4062),
// in the workspace otherwise; p in uint8 (n <= 255) or uint16; one barrier per k.  `<` on ascending t / k keeps the smallest index at
// ties (wave and block reductions compare the index explicitly); no atomics: bit-deterministic.  Penalty, argmin and backtrack run at
// the end of the same launch: no host synchronisation anywhere in the call.  The row scans, that tail, the markers and the per-video
// sizes are in kts_common.h, shared with the banded path (kts_banded.hip), which must return the same bits.
#include "kts_common.h"

namespace sumk {

namespace {
constexpr int KTS_MAX_N = 16384;
constexpr int KTS_THREADS = KTS_TAIL_THREADS;               // one block runs the DP rows and then the shared tail

struct KSeq {
  int64_t goff;    // fp32 Gram: element offset of the video's (n x ldg) block
  int64_t joff;    // float64 J / W and the caller's K blocks: element offset (sum of n^2)
  int64_t poff;    // p: byte offset
  int64_t ioff;    // I rows in the workspace: element offset (-1: the rows live in LDS)
  int32_t row0, n, ldg, m;   // first packed row, steps, Gram leading dimension, change points asked for = min(max_ncp, n - 1)
};

struct KtsWs { size_t gram, J, diag, p, irows, sc, seq, prob, total; int32_t n_max, tiles, nprob, lds; };

int kts_carve(int D, int n_seq, const int32_t* off, int max_ncp, bool want_gram, KtsWs* w) {
  SUMK_ARG(D > 0 && D % 4 == 0, "kts: D=%d must be a positive multiple of 4", D);
  SUMK_ARG(n_seq > 0 && off && off[0] == 0, "kts: empty batch");
  size_t g = 0, j = 0, pb = 0, ir = 0; int n_max = 0, tiles = 0, nprob = 0, lds = KTS_RED_BYTES;
  for (int s = 0; s < n_seq; ++s) {
    const int64_t n = (int64_t)off[s + 1] - off[s];
    SUMK_ARG(n >= 1 && n <= KTS_MAX_N, "kts: video %d has %lld steps (1 .. %d supported)", s, (long long)n, KTS_MAX_N);
    n_max = n > n_max ? (int)n : n_max;
  }
  SUMK_ARG(max_ncp >= 0 && max_ncp <= n_max - 1, "kts: max_ncp=%d outside 0 .. %d (longest video - 1)", max_ncp, n_max - 1);
  for (int s = 0; s < n_seq; ++s) {
    const KtsSizes z = kts_sizes(off[s + 1] - off[s], max_ncp);
    g += z.gram; j += z.J; pb += z.p; ir += z.irows;
    lds = z.lds > lds ? z.lds : lds;
    tiles += z.tiles; nprob += z.probs;
  }
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  w->gram = take(want_gram ? g * 4 : 0);
  w->J = take(j * 8);
  w->diag = take((size_t)off[n_seq] * 8);
  w->p = take(pb);
  w->irows = take(ir * 8);
  w->sc = take((size_t)n_seq * (max_ncp + 1) * 8);
  w->seq = take((size_t)n_seq * sizeof(KSeq));
  w->prob = take(want_gram ? (size_t)nprob * sizeof(GemmProb) : 0);
  w->total = p; w->n_max = n_max; w->tiles = tiles; w->nprob = nprob; w->lds = lds;
  return SUMK_OK;
}
}  // namespace

// One thread per video: its offsets (the sums of kts_sizes over the videos before it, as kts_carve adds them), and (features path) one
// GEMM problem per 64-row strip of its Gram matrix that covers the tiles from the diagonal to the right edge -- the tiles below the
// diagonal are never read and never computed.
__global__ void kts_setup_kernel(const int32_t* off, int n_seq, int D, int max_ncp, KSeq* seq, GemmProb* prob) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  int64_t goff = 0, joff = 0, poff = 0, ioff = 0; int ts = 0, pi = 0;
  for (int q = 0; q < s; ++q) {
    const KtsSizes z = kts_sizes(off[q + 1] - off[q], max_ncp);
    goff += z.gram; joff += z.J; poff += z.p; ioff += z.irows;
    ts += z.tiles; pi += z.probs;
  }
  const int row0 = off[s], n = off[s + 1] - row0;
  const KtsSizes z = kts_sizes(n, max_ncp);
  KSeq k; k.goff = goff; k.joff = joff; k.poff = poff; k.ioff = z.irows ? ioff : -1;
  k.row0 = row0; k.n = n; k.ldg = z.ldg; k.m = z.m;
  seq[s] = k;
  if (!prob) return;
  for (int r = 0; r < z.probs; ++r)
    ts += kts_strip_prob(prob + pi + r, row0, n, r, D, n - 64 * r, goff + (int64_t)64 * r * z.ldg + 64 * r, z.ldg, ts);
}

// Column pass: thread = column j, s descending from the diagonal.  FROM_F32: the symmetric fp32 Gram (upper triangle); otherwise the
// caller's float64 K, both triangles (any kernel matrix: symmetry is not assumed).
template <bool FROM_F32>
__global__ __launch_bounds__(256) void kts_col_kernel(const float* __restrict__ G, const double* __restrict__ Kd, const KSeq* __restrict__ seq,
                                                      double* __restrict__ W, double* __restrict__ diag) {
  const KSeq si = seq[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x, n = si.n;
  if (j >= n) return;
  const float* g = G + si.goff; const double* kd = Kd + si.joff;
  double* w = W + si.joff;
  const double d = FROM_F32 ? (double)g[(int64_t)j * si.ldg + j] : kd[(int64_t)j * n + j];
  diag[si.row0 + j] = d;
  w[(int64_t)j * n + j] = d;
  double acc = d;
#pragma unroll 4
  for (int s = j - 1; s >= 0; --s) {
    acc += FROM_F32 ? 2.0 * (double)g[(int64_t)s * si.ldg + j] : kd[(int64_t)s * n + j] + kd[(int64_t)j * n + s];
    w[(int64_t)s * n + j] = acc;
  }
}

// Row pass: one wave per row i; kts_row_scan over t = i .. n - 1, J over W.
__global__ __launch_bounds__(256) void kts_row_kernel(const KSeq* __restrict__ seq, double* __restrict__ W, const double* __restrict__ diag) {
  const KSeq si = seq[blockIdx.y];
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), n = si.n;
  if (i >= n) return;
  kts_row_scan(W + si.joff + (int64_t)i * n + i, diag + si.row0 + i, n - i, threadIdx.x & 63);
}

struct KtsArgs {
  const KSeq* seq; const double* J; void* p; double* irows; double* sc;
  int32_t max_ncp, lmin, lmax, fixed_m; double vmax;
  int32_t* n_cps; int32_t* cps; double* scores;
};

__device__ __forceinline__ int kts_p_load(const void* p, bool narrow, int64_t idx) {
  return narrow ? (int)((const uint8_t*)p)[idx] : (int)((const uint16_t*)p)[idx];
}

// The m dependent steps of one video.  I0 / I1 are both in LDS or both in the workspace (one inlined copy per address space).
__device__ __forceinline__ void kts_dp_rows(double* I0, double* I1, const double* __restrict__ J, void* p, bool narrow, double* __restrict__ sc,
                                            int n, int m, int lmin, int lmax) {
  const int tid = threadIdx.x;
  for (int l = tid; l <= n; l += KTS_THREADS) I0[l] = (l >= lmin && l < lmax) ? J[l - 1] : KTS_BIG;   // (lmax is EXCLUSIVE here: kept quirk)
  __syncthreads();
  if (tid == 0) sc[0] = I0[n];
  double* prev = I0; double* cur = I1;
  int k = 1;
  for (; k <= m; ++k) {
    const int64_t lstart = (int64_t)(k + 1) * lmin;
    if (lstart > n) break;                                   // rows k .. m have no feasible end point (uniform over the block)
    const int tlo = (int)((int64_t)k * lmin);
    for (int l = (int)lstart + tid; l <= n; l += KTS_THREADS) {
      const int t0 = l - lmax > tlo ? l - lmax : tlo;
      const double* jc = J + (l - 1);
      double best = INFINITY; int arg = t0;
#pragma unroll 8
      for (int t = t0; t < l; ++t) {
        const double c = prev[t] + jc[(int64_t)t * n];
        if (c < best) { best = c; arg = t; }                  // ascending t and a strict compare: the smallest t wins a tie
      }
      cur[l] = best;
      const int64_t pi = (int64_t)(k - 1) * (n + 1) + l;
      if (narrow) ((uint8_t*)p)[pi] = (uint8_t)arg; else ((uint16_t*)p)[pi] = (uint16_t)arg;
      if (l == n) sc[k] = best;
    }
    __syncthreads();
    double* t = prev; prev = cur; cur = t;
  }
  for (int q = k + tid; q <= m; q += KTS_THREADS) sc[q] = KTS_BIG;
  __syncthreads();
}

__global__ __launch_bounds__(KTS_THREADS) void kts_dp_kernel(KtsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double kts_lds[];
  const int v = blockIdx.x;
  const KSeq si = a.seq[v];
  const int n = si.n, m = si.m;
  const bool narrow = kts_p_narrow(n);
  const double* J = a.J + si.joff;
  void* p = (char*)a.p + si.poff;
  double* sc = a.sc + (int64_t)v * (a.max_ncp + 1);
  double* red;
  if (si.ioff < 0) {
    kts_dp_rows(kts_lds, kts_lds + (n + 1), J, p, narrow, sc, n, m, a.lmin, a.lmax);
    red = kts_lds + 2 * (n + 1);
  } else {
    double* I0 = a.irows + si.ioff;
    kts_dp_rows(I0, I0 + (n + 1), J, p, narrow, sc, n, m, a.lmin, a.lmax);
    red = kts_lds;
  }
  const KtsTail t = {a.max_ncp, a.lmin, a.fixed_m, a.vmax, a.n_cps, a.cps, a.scores};
  kts_tail(t, v, n, m, sc, red, (int*)(red + 16), [&](int64_t idx) { return kts_p_load(p, narrow, idx); });
}

static int kts_run(const float* x, const double* K, int D, int n_seq, const int32_t* off_host, const int32_t* off_dev, int max_ncp, int lmin,
                   int lmax, double vmax, int fixed_m, int32_t* n_cps, int32_t* cps, double* scores, void* workspace, size_t workspace_bytes,
                   hipStream_t stream, const char* who) {
  SUMK_TRY(kts_check_args(who, x ? (const void*)x : (const void*)K, off_dev, n_cps, cps, workspace, max_ncp, lmin, lmax, vmax));
  KtsWs L;
  SUMK_TRY(kts_carve(D, n_seq, off_host, max_ncp, x != nullptr, &L));
  SUMK_ARG(workspace_bytes >= L.total, "%s: workspace %zu < required %zu", who, workspace_bytes, L.total);
  char* ws = (char*)workspace;
  float* G = (float*)(ws + L.gram);
  double* W = (double*)(ws + L.J);
  double* diag = (double*)(ws + L.diag);
  KSeq* seq = (KSeq*)(ws + L.seq);
  GemmProb* prob = x ? (GemmProb*)(ws + L.prob) : nullptr;
  hipLaunchKernelGGL(kts_setup_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, off_dev, n_seq, D, max_ncp, seq, prob);
  const dim3 cgrid((L.n_max + 255) / 256, n_seq), rgrid((L.n_max + 3) / 4, n_seq);
  if (x) {
    GemmLaunch g;
    g.A = x; g.B[0] = x; g.C = G; g.probs = prob; g.nprob = L.nprob; g.small_tile = 1; g.total_tiles = L.tiles;
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_NONE, g, stream));
    hipLaunchKernelGGL(kts_col_kernel<true>, cgrid, dim3(256), 0, stream, G, (const double*)nullptr, seq, W, diag);
  } else {
    hipLaunchKernelGGL(kts_col_kernel<false>, cgrid, dim3(256), 0, stream, (const float*)nullptr, K, seq, W, diag);
  }
  hipLaunchKernelGGL(kts_row_kernel, rgrid, dim3(256), 0, stream, seq, W, diag);
  KtsArgs a;
  a.seq = seq; a.J = W; a.p = ws + L.p; a.irows = (double*)(ws + L.irows); a.sc = (double*)(ws + L.sc);
  a.max_ncp = max_ncp; a.lmin = lmin; a.lmax = lmax; a.fixed_m = fixed_m; a.vmax = vmax;
  a.n_cps = n_cps; a.cps = cps; a.scores = scores;
  hipLaunchKernelGGL(kts_dp_kernel, dim3(n_seq), dim3(KTS_THREADS), (size_t)L.lds, stream, a);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_kts_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t max_ncp) {
  KtsWs w;
  if (kts_carve(D, n_seq, seq_off_host, max_ncp, true, &w) != SUMK_OK) return 0;
  return w.total;
}

extern "C" int sumk_kts(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, int32_t max_ncp,
                        int32_t lmin, int32_t lmax, double vmax, int32_t* n_cps, int32_t* cps, double* scores, void* workspace,
                        size_t workspace_bytes, void* stream) {
  SUMK_ARG(x, "kts: null features");
  return kts_run(x, nullptr, D, n_seq, seq_off_host, seq_off_dev, max_ncp, lmin, lmax, vmax, 0, n_cps, cps, scores, workspace, workspace_bytes,
                 (hipStream_t)stream, "kts");
}

extern "C" int sumk_kts_gram(const double* K, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, int32_t max_ncp,
                             int32_t lmin, int32_t lmax, double vmax, int32_t* n_cps, int32_t* cps, double* scores, void* workspace,
                             size_t workspace_bytes, void* stream) {
  SUMK_ARG(K, "kts_gram: null kernel matrices");
  return kts_run(nullptr, K, 4, n_seq, seq_off_host, seq_off_dev, max_ncp, lmin, lmax, vmax, 0, n_cps, cps, scores, workspace, workspace_bytes,
                 (hipStream_t)stream, "kts_gram");
}

extern "C" int sumk_kts_gram_nonlin(const double* K, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, int32_t ncp,
                                    int32_t lmin, int32_t lmax, int32_t* n_cps, int32_t* cps, double* scores, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  SUMK_ARG(K, "kts_gram_nonlin: null kernel matrices");
  return kts_run(nullptr, K, 4, n_seq, seq_off_host, seq_off_dev, ncp, lmin, lmax, 1.0, 1, n_cps, cps, scores, workspace, workspace_bytes,
                 (hipStream_t)stream, "kts_gram_nonlin");
}
