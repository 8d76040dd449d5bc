// What the dense (kts.hip) and the banded (kts_banded.hip) change-point paths share.  Both must return the same n_cps, cps and the same
// BITS of scores (tests/test_gpu_kts_banded.py), so everything that decides those bits and is not tied to one storage layout exists once,
// here: the markers, the row scans that turn W into J, and the tail (penalty, arg-min over k, backtrack, score row).  Each path also
// carves its workspace on the host and hands every video its offsets on the device; the two sides must agree byte for byte, so the
// per-video sizes come from one __host__ __device__ function per path, called by both.
#pragma once
#include "sumk_internal.h"
#include <math.h>

namespace sumk {

constexpr int KTS_TAIL_THREADS = 1024;
constexpr int KTS_RED_BYTES = 512;                          // dense path: block-reduction scratch behind the two I rows in LDS
constexpr int KTS_LDS_LIMIT = 65536;
constexpr double KTS_BIG = 1e101, KTS_INF_ABOVE = 1e99;     // "no segmentation" marker of the original code and its reporting threshold

// ---- per-video sizes.  gram / J / irows count elements (float, double, double); p counts bytes on the dense path (uint8 or uint16 table)
// and int32 elements on the banded one; tiles / probs are the 64x64 tiles and the 64-row strips of the video's Gram launch.
struct KtsSizes {
  int64_t gram, J, p, irows;         // irows == 0: the two I rows live in LDS (dense path only), lds = their bytes + KTS_RED_BYTES
  int32_t tiles, probs, lds, ldg, m; // Gram leading dimension; change points asked for = min(max_ncp, n - 1)
};
struct KtsBandSizes : KtsSizes { int32_t B; };     // band width min(lmax, n)

__host__ __device__ inline bool kts_p_narrow(int n) { return n <= 255; }      // dense p table: uint8, else uint16

__host__ __device__ inline KtsSizes kts_sizes(int n, int max_ncp) {
  const int64_t n1 = (int64_t)n + 1, rows_lds = 2 * n1 * 8 + KTS_RED_BYTES;
  const int tm = (n + 63) / 64;
  KtsSizes z;
  z.m = max_ncp < n - 1 ? max_ncp : n - 1; z.ldg = (n + 3) & ~3;
  z.gram = (int64_t)n * z.ldg; z.J = (int64_t)n * n;
  z.p = ((int64_t)z.m * n1 * (kts_p_narrow(n) ? 1 : 2) + 15) / 16 * 16;
  z.irows = rows_lds <= KTS_LDS_LIMIT ? 0 : 2 * n1; z.lds = z.irows ? 0 : (int)rows_lds;
  z.tiles = tm * (tm + 1) / 2; z.probs = tm;              // the tiles on and above the diagonal
  return z;
}

// columns of strip r (rows 64 r .. 64 r + 63) of the banded Gram: from its own diagonal column 64 r to the last one a band of B reaches
__host__ __device__ inline int kts_band_strip_n(int n, int B, int r) { return n - 64 * r < B + 63 ? n - 64 * r : B + 63; }

__host__ __device__ inline KtsBandSizes kts_band_sizes(int n, int max_ncp, int lmax) {
  const int64_t n1 = (int64_t)n + 1;
  KtsBandSizes z;
  z.B = lmax < n ? lmax : n;
  z.m = max_ncp < n - 1 ? max_ncp : n - 1; z.ldg = (kts_band_strip_n(n, z.B, 0) + 3) & ~3;
  z.gram = (int64_t)n * z.ldg; z.J = (int64_t)n * z.B;
  z.p = ((int64_t)z.m * n1 + 3) / 4 * 4;
  z.irows = 2 * n1; z.lds = 0;
  z.probs = (n + 63) / 64; z.tiles = 0;
  for (int r = 0; r < z.probs; ++r) z.tiles += (kts_band_strip_n(n, z.B, r) + 63) / 64;
  return z;
}

// The GemmProb of one 64-row strip of a video's Gram matrix X X^T: rows 64 r .. of the video (first packed row row0, n steps) against the N
// rows that start at the same row, written at c_off with leading dimension ldc.  Returns the strip's tiles.
__device__ inline int kts_strip_prob(GemmProb* out, int row0, int n, int r, int D, int N, int64_t c_off, int ldc, int tile_start) {
  GemmProb q;
  q.a_off = (int64_t)(row0 + 64 * r) * D; q.b_off = q.a_off; q.c_off = c_off; q.r_off = 0;
  q.M = n - 64 * r < 64 ? n - 64 * r : 64; q.N = N; q.K = D; q.lda = D; q.ldb = D; q.ldc = ldc; q.ldr = 0;
  q.tile_start = tile_start; q.tiles_n = (N + 63) / 64;
  for (int i = 0; i < 7; ++i) q.pad_[i] = 0;
  *out = q;
  return q.tiles_n;
}

// ---- argument checks of the run entry points (`who` = the prefix of every message)
inline int kts_check_args(const char* who, const void* src, const void* off_dev, const void* n_cps, const void* cps, const void* workspace,
                          int max_ncp, int lmin, int lmax, double vmax) {
  SUMK_ARG(src && off_dev && n_cps && workspace, "%s: null pointer", who);
  SUMK_ARG(cps || max_ncp == 0, "%s: null cps", who);
  SUMK_ARG(lmin >= 1 && lmax >= lmin, "%s: need 1 <= lmin <= lmax, got lmin=%d lmax=%d", who, lmin, lmax);
  SUMK_ARG(vmax == vmax, "%s: vmax is NaN", who);
  return SUMK_OK;
}

// ---- row pass: one wave per row.  Inclusive scans of w[c] (the column-pass increments W[i][i + c]) and dg[c] (K[i + c][i + c]) over
// c = 0 .. len - 1 in chunks of 64 with a carry; J[i][i + c] = d - a / (c + 1) written over w[c].
__device__ __forceinline__ void kts_row_scan(double* w, const double* dg, int len, int lane) {
  double cs = 0.0, cd = 0.0;
  for (int base = 0; base < len; base += 64) {
    const int c = base + lane;
    double a = c < len ? w[c] : 0.0, d = c < len ? dg[c] : 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double ua = __shfl_up(a, o), ud = __shfl_up(d, o);
      if (lane >= o) { a += ua; d += ud; }
    }
    a += cs; d += cd;
    if (c < len) w[c] = d - a / (double)(c + 1);
    cs = __shfl(a, 63); cd = __shfl(d, 63);
  }
}

// ---- tail of one video, run by a block of KTS_TAIL_THREADS: penalty + arg-min over k (unless fixed_m), backtrack through p, score row.
// sc[0 .. m] = I[k][n] (KTS_BIG where the DP had no feasible end point), red / redk = 16 doubles / 16 ints of LDS, p_at(idx) = entry idx of
// the video's p table, row k - 1 at (k - 1) (n + 1).  Every thread of the block must call it (barriers inside).
struct KtsTail {
  int32_t max_ncp, lmin, fixed_m; double vmax;
  int32_t* n_cps; int32_t* cps; double* scores;
};

template <class P>
__device__ __forceinline__ void kts_tail(const KtsTail& a, int v, int n, int m, const double* sc, double* red, int* redk, P p_at) {
  const int tid = threadIdx.x;
  // the smallest k at a tie; an infinite score never wins: +inf < x is false and k = 0 is the start value
  int mb = m;
  if (!a.fixed_m) {
    double best = INFINITY; int bk = 0;
    for (int k = tid; k <= m; k += KTS_TAIL_THREADS) {
      double s = sc[k];
      if (s > KTS_INF_ABOVE) s = INFINITY;
      double c = s / (double)n;
      if (k > 0) c += (a.vmax * (double)k / (2.0 * (double)n)) * (log((double)n / (double)k) + 1.0);
      if (c < best) { best = c; bk = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o); const int ok = __shfl_xor(bk, o);
      if (ob < best || (ob == best && ok < bk)) { best = ob; bk = ok; }
    }
    if ((tid & 63) == 0) { red[tid >> 6] = best; redk[tid >> 6] = bk; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < KTS_TAIL_THREADS / 64; ++w)
        if (red[w] < best || (red[w] == best && redk[w] < bk)) { best = red[w]; bk = redk[w]; }
      redk[0] = best < INFINITY ? bk : 0;
    }
    __syncthreads();
    mb = redk[0];
  }
  if (tid == 0) {
    a.n_cps[v] = mb;
    int32_t* out = a.cps + (int64_t)v * a.max_ncp;
    int cur = n;
    for (int k = mb; k >= 1; --k) {
      // an entry the DP never wrote (no feasible end point there) reads as 0, as in the zero-initialised table of the original
      cur = cur >= (int64_t)(k + 1) * a.lmin ? p_at((int64_t)(k - 1) * (n + 1) + cur) : 0;
      out[k - 1] = cur;
    }
    for (int k = mb; k < a.max_ncp; ++k) out[k] = -1;
  }
  if (a.scores) {
    double* so = a.scores + (int64_t)v * (a.max_ncp + 1);
    for (int k = tid; k <= a.max_ncp; k += KTS_TAIL_THREADS) {
      double s = INFINITY;
      if (k <= mb) { s = sc[k]; if (s > KTS_INF_ABOVE) s = INFINITY; }
      so[k] = s;
    }
  }
}

}  // namespace sumk
