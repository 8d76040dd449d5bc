// DSN diversity-representativeness reward WITHOUT the Gram matrix: the streaming form of csrc/reward.hip for long videos.
//
// reward.hip stores G = X X^T per video (T x T floats: 17 GB at T = 65 536) and reads a whole row of it per (episode, frame).  Every
// element G[t][p] is used once per episode -- in a row minimum over the picks, d2 = G[t][t] + G[p][p] - 2 G[t][p], and for a picked t in
// a row sum of 1 - cos or of the constant 1 -- so here it is consumed in registers the moment the MFMA accumulators hold it: the Gram
// tile is never stored and all episodes of a chunk are served from one pass over the tiles.  Workspace is O(E x n_rows).
//
// Launches of one call (all on the caller's stream, nothing else: the call captures into a HIP graph):
//   rs_setup_kernel   per-video descriptors (tile / block / row-block prefix sums) from the device offsets
//   rs_bits_kernel    pick bits: one 64-bit ballot per (episode, 64-column tile); a video's columns are padded to 64 with zero bits
//   rs_norm_kernel    the Gram on the ceil(T / 64) DIAGONAL tiles only, keeping their diagonals: sq[t] = G[t][t] comes out of the same
//                     MFMA sequence the streaming pass runs, so G[t][t] there has the bits of sq[t] and d2(t, t) is exactly 0
//   per chunk of EC episodes:
//     rs_stream_kernel  one workgroup per (video, 64-row strip, column split): walks its share of the 64-column key tiles in ascending
//                       order (every strip in the same order: a key tile is shared through L2 by the strips running at that time).  The
//                       k-loop per tile is that of gemm_lean_kernel<true> (NT, buffer loads, scalar k advance).  The KEY tile is the MFMA's
//                       A operand and the query strip its B operand: a lane owns ONE query row and 16 keys per 32 x 32 sub-tile, so the
//                       per-episode reductions are register arithmetic without cross-lane traffic.  A key tile with no pick in any
//                       episode of the chunk contributes nothing and its k-loop is skipped.  At the end of the walk the two lane halves
//                       and the two waves that share a row are joined in a fixed order: one partial per (episode, row, split).
//     rs_rows_kernel    per (episode, 1024 rows): the splits of a row joined in split order, rows summed in a fixed order
//     rs_join_kernel    per (episode, video): row-block partials in block order, pick count, the reward
// No cooperative launch, no flag polled across workgroups, no float atomics: bit-deterministic.
#include "gemm_device.h"
#include <math.h>
#include <algorithm>

namespace sumk {

typedef unsigned int rs_u32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int RT = 64, RBK = 32;                 // tile edge, k-tile
constexpr int RPITCH = RBK + 4;                  // K-contiguous LDS image: [row][RBK + 4] floats (conflict-free ds_read_b128)
constexpr int RIMG = RT * RPITCH;                // one operand image: 2304 floats
constexpr int RSTAGE = 2 * RIMG;                 // key image + query image
constexpr int RS_EC = 8;                         // episodes per pass (sumk.h: SUMK_REWARD_STREAM_EC)
constexpr int RS_MAX_SPLIT = 8;
constexpr int RS_MAX_T = 1 << 20;
constexpr int RS_RB_TILES = 16;                  // a row block of rs_rows_kernel: 16 tiles = 1024 rows
static_assert(RS_EC == SUMK_REWARD_STREAM_EC, "sumk.h names the chunk");
static_assert(2 * RSTAGE >= 256 * 3 * RS_EC, "the end-of-walk join re-uses the staging images");
}

struct RsSeq {
  int64_t row0;        // first packed row of the video
  int32_t T, tiles;    // frames, 64-row strips (= 64-column key tiles)
  int32_t tile0;       // first tile in the padded layouts (sq / rinv / partials: 64 tile0 + t, pick words: 2 tile0 + ...)
  int32_t S;           // column splits of this video: min(plan, tiles)
  int32_t blk0;        // first workgroup of rs_stream_kernel: blk0 + split * tiles + strip
  int32_t rb0, nrb;    // row blocks of rs_rows_kernel
  int32_t pad_;
};

struct RsWs { size_t seq, sq, rinv, bits, pmin, pcs, pcnt, bpart, total; int64_t tiles, rblocks; int32_t ec; };

struct RsBlockPart { float smin, scs; long long cnt; };

static int rs_carve(int D, int n_seq, const int32_t* off, int n_ep, RsWs* w) {
  SUMK_ARG(D > 0 && D % 4 == 0 && D <= (1 << 20), "dsn_reward_stream: D=%d must be a positive multiple of 4 (at most 1048576)", D);
  SUMK_ARG(n_seq > 0 && off && off[0] == 0 && n_ep > 0, "dsn_reward_stream: empty batch");
  int64_t tiles = 0, rblocks = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int T = off[s + 1] - off[s];
    SUMK_ARG(T > 0, "dsn_reward_stream: video %d has %d frames", s, T);
    SUMK_ARG(T <= RS_MAX_T, "dsn_reward_stream: video %d has %d frames (at most %d)", s, T, RS_MAX_T);
    const int tm = (T + RT - 1) / RT;
    tiles += tm; rblocks += (tm + RS_RB_TILES - 1) / RS_RB_TILES;
  }
  SUMK_ARG(tiles < (1 << 25), "dsn_reward_stream: %lld row strips in one call (at most 2^25)", (long long)tiles);
  const int ec = std::min(n_ep, RS_EC);
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  w->tiles = tiles; w->rblocks = rblocks; w->ec = ec;
  w->seq = take((size_t)n_seq * sizeof(RsSeq));
  w->sq = take((size_t)tiles * RT * 4);
  w->rinv = take((size_t)tiles * RT * 4);
  w->bits = take((size_t)n_ep * tiles * 2 * 4);
  const size_t part = (size_t)ec * RS_MAX_SPLIT * tiles * RT * 4;      // [episode of the chunk][split][padded row]
  w->pmin = take(part); w->pcs = take(part); w->pcnt = take(part);
  w->bpart = take((size_t)ec * rblocks * sizeof(RsBlockPart));
  w->total = p;
  return SUMK_OK;
}

// S so that strips x S is about one round of resident workgroups (4 per CU on 256 CUs); at most RS_MAX_SPLIT (the workspace is sized
// for that), and per video at most its column tiles (rs_setup_kernel)
static int rs_plan(int n_seq, const int32_t* off) {
  int64_t tiles = 0;
  for (int s = 0; s < n_seq; ++s) tiles += (off[s + 1] - off[s] + RT - 1) / RT;
  int64_t S = tiles > 0 ? (1024 + tiles / 2) / tiles : 1;
  return (int)std::max<int64_t>(1, std::min<int64_t>(S, RS_MAX_SPLIT));
}

__global__ void rs_setup_kernel(const int32_t* off, int n_seq, int S, RsSeq* seq) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  int tile0 = 0, blk0 = 0, rb0 = 0;
  for (int q = 0; q < s; ++q) {
    const int tm = (off[q + 1] - off[q] + RT - 1) / RT;
    tile0 += tm; blk0 += tm * min(S, tm); rb0 += (tm + RS_RB_TILES - 1) / RS_RB_TILES;
  }
  const int T = off[s + 1] - off[s], tm = (T + RT - 1) / RT;
  RsSeq d;
  d.row0 = off[s]; d.T = T; d.tiles = tm; d.tile0 = tile0; d.S = min(S, tm); d.blk0 = blk0; d.rb0 = rb0;
  d.nrb = (tm + RS_RB_TILES - 1) / RS_RB_TILES; d.pad_ = 0;
  seq[s] = d;
}

// the video whose range [first(s), first(s + 1)) holds `v` (first = one of the prefix sums of RsSeq); wave-uniform when v is
template <typename F>
__device__ __forceinline__ int rs_find(int n_seq, int v, F first) {
  int lo = 0, hi = n_seq - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first(mid) <= v) lo = mid; else hi = mid - 1; }
  return lo;
}

// one wave per (episode, tile): lane = column; bits[e][2 (tile0 + c)], [.. + 1] = the picks among columns 64 c .. 64 c + 63
__global__ __launch_bounds__(256) void rs_bits_kernel(const float* __restrict__ actions, const RsSeq* __restrict__ seq, int n_seq,
                                                      int n_tiles, int n_ep, int64_t n_rows, unsigned* __restrict__ bits) {
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (int64_t)n_ep * n_tiles) return;
  const int lane = threadIdx.x & 63;
  const int e = (int)(wid / n_tiles), tile = (int)(wid % n_tiles);
  const RsSeq d = seq[rs_find(n_seq, tile, [&](int q) { return seq[q].tile0; })];
  const int t = (tile - d.tile0) * RT + lane;
  const bool pick = t < d.T && actions[(int64_t)e * n_rows + d.row0 + t] != 0.f;
  const unsigned long long b = __ballot(pick);
  if (lane == 0) {
    bits[((int64_t)e * n_tiles + tile) * 2] = (unsigned)b;
    bits[((int64_t)e * n_tiles + tile) * 2 + 1] = (unsigned)(b >> 32);
  }
}

// ---- one 64 x 64 Gram tile: acc = keys (A operand) x queries (B operand) over D, k ascending -- the k-loop of gemm_lean_kernel<true>.
// Called by all 256 threads; ends behind a barrier (the images are free again).  Wave (wk, wq) holds keys 32 wk + (r & 3) + 8 (r >> 2) +
// 4 (lane >> 5), query 32 wq + (lane & 31) in acc[r].  Rows past krows / qrows are clamped to the last valid row: they feed only
// columns whose pick bit is zero and rows that are never stored.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rs_rsrc(const float* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), (short)0, 0x7FFFFFFF, 0x00020000);
}

__device__ __forceinline__ void rs_gram_tile(const float* __restrict__ Kbase, int krows, const float* __restrict__ Qbase, int qrows, int D,
                                             float* lds, bool live, f32x16& acc) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wave >> 1, wq = wave & 1, li = lane & 31, lh = lane >> 5;
  const int kq = (tid & 7) * 4;
  const int nk = (D + RBK - 1) / RBK;
  const bool has_tail = (D % RBK) != 0;
  int voK[2], voQ[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    voK[p] = (min((tid >> 3) + 32 * p, krows - 1) * D + kq) * 4;
    voQ[p] = (min((tid >> 3) + 32 * p, qrows - 1) * D + kq) * 4;
  }
  float4 ra[2], rb[2];
  auto as4 = [](rs_u32x4 v) { return __builtin_bit_cast(float4, v); };
  const __amdgpu_buffer_rsrc_t sK = rs_rsrc(Kbase), sQ = rs_rsrc(Qbase);
  auto gload = [&](int kt) {                       // a full k-tile: the k advance is the scalar offset
#pragma unroll
    for (int p = 0; p < 2; ++p) ra[p] = as4(__builtin_amdgcn_raw_buffer_load_b128(sK, voK[p], kt * (RBK * 4), 0));
#pragma unroll
    for (int p = 0; p < 2; ++p) rb[p] = as4(__builtin_amdgcn_raw_buffer_load_b128(sQ, voQ[p], kt * (RBK * 4), 0));
  };
  auto gload_tail = [&](int kt) {                  // D % 32 != 0: D % 4 == 0, so a float4 lies wholly inside or outside the row
    const int k = kt * RBK + kq;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int rK = min((tid >> 3) + 32 * p, krows - 1), rQ = min((tid >> 3) + 32 * p, qrows - 1);
      ra[p] = k < D ? *reinterpret_cast<const float4*>(Kbase + (int64_t)rK * D + k) : z;
      rb[p] = k < D ? *reinterpret_cast<const float4*>(Qbase + (int64_t)rQ * D + k) : z;
    }
  };
  auto gload_any = [&](int kt) { if (has_tail && kt == nk - 1) gload_tail(kt); else gload(kt); };

  const int wA = (tid >> 3) * RPITCH + kq;
  const int wB = RIMG + wA;
  const int fA = (wk * 32 + li) * RPITCH + 4 * lh;
  const int fB = RIMG + (wq * 32 + li) * RPITCH + 4 * lh;
  auto swrite = [&](float* img) {
    *reinterpret_cast<float4*>(img + wA) = ra[0];
    *reinterpret_cast<float4*>(img + wA + 32 * RPITCH) = ra[1];
    *reinterpret_cast<float4*>(img + wB) = rb[0];
    *reinterpret_cast<float4*>(img + wB + 32 * RPITCH) = rb[1];
  };
  // fragments of HALF a k-tile (2 x float4 of each operand per lane): the per-episode running values leave no room for a whole one
  float fa[2][4], fb[2][4];
  auto read_frags = [&](const float* img, int h) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(img + fA + 8 * (2 * h + q));
      fa[q][0] = a.x; fa[q][1] = a.y; fa[q][2] = a.z; fa[q][3] = a.w;
      const float4 b = *reinterpret_cast<const float4*>(img + fB + 8 * (2 * h + q));
      fb[q][0] = b.x; fb[q][1] = b.y; fb[q][2] = b.z; fb[q][3] = b.w;
    }
  };
  auto mfma_half = [&]() {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][j], fb[q][j], acc, 0, 0, 0);
  };

  float* im0 = lds;
  float* im1 = lds + RSTAGE;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  gload_any(0);
  swrite(im0);
  if (nk > 1) gload_any(1);
  __syncthreads();
  // steady state, unrolled by two (image addresses are immediates): k-tiles kt whose kt + 2 is a FULL k-tile
  const int n_steady = has_tail ? nk - 3 : nk - 2;
  int kt = 0;
  auto step = [&](float* cur_img, float* oth_img, int kt_) {
    if (live) { read_frags(cur_img, 0); mfma_half(); }
    swrite(oth_img);
    if (live) { read_frags(cur_img, 1); mfma_half(); }
    gload(kt_ + 2);
    __syncthreads();
  };
  for (; kt + 1 < n_steady; kt += 2) {
    step(im0, im1, kt);
    step(im1, im0, kt + 1);
  }
  float* cur_img = im0; float* oth_img = im1;     // kt is even here
  for (; kt < nk; ++kt) {
    if (live) { read_frags(cur_img, 0); mfma_half(); }
    if (kt + 1 < nk) swrite(oth_img);
    if (live) { read_frags(cur_img, 1); mfma_half(); }
    if (kt + 2 < nk) gload_any(kt + 2);
    __syncthreads();
    float* t = cur_img; cur_img = oth_img; oth_img = t;
  }
}

// one workgroup per tile: the diagonal Gram tile, its diagonal -> sq, 1 / sqrt -> rinv (all 64 positions of the tile are written; the
// positions past T repeat the last row and are never read through a set pick bit)
__global__ __launch_bounds__(256, 4) void rs_norm_kernel(const float* __restrict__ x, int D, const RsSeq* __restrict__ seq, int n_seq,
                                                         float* __restrict__ sq, float* __restrict__ rinv) {
  __shared__ __attribute__((aligned(16))) float lds[2 * RSTAGE];
  const int tile = blockIdx.x;
  const RsSeq d = seq[rs_find(n_seq, tile, [&](int q) { return seq[q].tile0; })];
  const int c = tile - d.tile0, rows = min(RT, d.T - c * RT);
  const float* base = x + (d.row0 + (int64_t)c * RT) * D;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wk = wave >> 1, wq = wave & 1, li = lane & 31, lh = lane >> 5;
  f32x16 acc;
  rs_gram_tile(base, rows, base, rows, D, lds, wk == wq, acc);       // the off-diagonal waves only stage
  if (wk == wq && lh == ((li >> 2) & 1)) {          // key 8 (li >> 3) + 4 lh + (li & 3) == query li: r = 4 (li >> 3) + (li & 3)
    const int rsel = 4 * (li >> 3) + (li & 3);
    float g = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) g = r == rsel ? acc[r] : g;
    const int64_t pos = (int64_t)tile * RT + wq * 32 + li;
    sq[pos] = g;
    rinv[pos] = 1.0f / sqrtf(g);
  }
}

struct RsStreamArgs {
  const float* x; const RsSeq* seq; const unsigned* bits; const float* sq; const float* rinv;
  float* pmin; float* pcs; int* pcnt;
  int32_t D, n_seq, n_tiles, e0, ne, far_sim, thre;
};

__global__ __launch_bounds__(256, 4) void rs_stream_kernel(RsStreamArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[2 * RSTAGE];
  const int blk = blockIdx.x;
  const RsSeq d = a.seq[rs_find(a.n_seq, blk, [&](int q) { return a.seq[q].blk0; })];
  const int local = blk - d.blk0, split = local / d.tiles, strip = local % d.tiles;
  const int c_lo = (int)((int64_t)split * d.tiles / d.S), c_hi = (int)((int64_t)(split + 1) * d.tiles / d.S);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wave >> 1, wq = wave & 1, li = lane & 31, lh = lane >> 5;
  const int qrows = min(RT, d.T - strip * RT);
  const float* Qbase = a.x + (d.row0 + (int64_t)strip * RT) * a.D;
  const int t = strip * RT + wq * 32 + li;                       // this lane's query row inside the video
  const int64_t qpos = (int64_t)(d.tile0 + strip) * RT + wq * 32 + li;
  const float sqt = a.sq[qpos], rit = a.rinv[qpos];
  // pick words: episode e of the chunk, tile c, half h -> bits[(e0 + e) n_tiles 2 + 2 (tile0 + c) + h]
  const unsigned* bw = a.bits + ((int64_t)a.e0 * a.n_tiles + d.tile0) * 2;
  const int64_t estride = (int64_t)a.n_tiles * 2;
  unsigned pqm = 0u;                               // bit e: this lane's query row is picked in episode e of the chunk
  float mn[RS_EC], cs[RS_EC];
  int cnt[RS_EC];
#pragma unroll
  for (int e = 0; e < RS_EC; ++e) {
    const unsigned w = e < a.ne ? bw[e * estride + 2 * strip + wq] : 0u;
    pqm |= ((w >> li) & 1u) << e;
    mn[e] = INFINITY; cs[e] = 0.f; cnt[e] = 0;
  }
  const bool use_thre = !a.far_sim;

  for (int c = c_lo; c < c_hi; ++c) {
    // a key tile without a pick in any episode of the chunk contributes nothing (workgroup-uniform)
    unsigned any = 0u;
#pragma unroll
    for (int e = 0; e < RS_EC; ++e)
      if (e < a.ne) any |= bw[e * estride + 2 * c] | bw[e * estride + 2 * c + 1];
    if (any == 0u) continue;
    const int krows = min(RT, d.T - c * RT);
    const bool live = (wk * 32 < krows) && (wq * 32 < qrows);
    f32x16 acc;
    rs_gram_tile(a.x + (d.row0 + (int64_t)c * RT) * a.D, krows, Qbase, qrows, a.D, lds, live, acc);
    unsigned kw[RS_EC], wany = 0u;                                // this wave's 32 keys (scalar loads, read again behind the k-loop)
#pragma unroll
    for (int e = 0; e < RS_EC; ++e) { kw[e] = e < a.ne ? bw[e * estride + 2 * c + wk] : 0u; wany |= kw[e]; }
    if (!live || wany == 0u) continue;                           // wave-uniform: no pick among this wave's 32 keys
    const int kbase = c * RT + wk * 32;                          // first key of the sub-tile inside the video
    const float* sqk = a.sq + (int64_t)(d.tile0 + c) * RT + wk * 32 + 4 * lh;
    const float* rik = a.rinv + (int64_t)(d.tile0 + c) * RT + wk * 32 + 4 * lh;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const float4 s4 = *reinterpret_cast<const float4*>(sqk + 8 * q4);
      const float4 r4 = *reinterpret_cast<const float4*>(rik + 8 * q4);
      const float sv[4] = {s4.x, s4.y, s4.z, s4.w}, rv[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float g = acc[4 * q4 + b];
        const int kl = 8 * q4 + 4 * lh + b;                      // key inside the sub-tile = its bit in the pick word
        const float d2 = (sqt + sv[b]) - 2.f * g;
        const float dc = 1.f - g * rit * rv[b];
        const int p = kbase + kl;
        const int dist = t > p ? t - p : p - t;
        const bool far = use_thre && dist > a.thre;
#pragma unroll
        for (int e = 0; e < RS_EC; ++e) {
          const bool pk = (kw[e] >> kl) & 1u;
          mn[e] = pk ? fminf(mn[e], d2) : mn[e];
          const bool pair = pk && ((pqm >> e) & 1u);
          cnt[e] += (pair && far) ? 1 : 0;
          cs[e] = (pair && !far) ? cs[e] + dc : cs[e];
        }
      }
    }
  }

  // ---- join: ((wk 0: lh 0, lh 1), (wk 1: lh 0, lh 1)) in that order, through the staging images (free behind the tile's last barrier)
  __syncthreads();
  float* red = lds;                                // [thread][3 RS_EC]
#pragma unroll
  for (int e = 0; e < RS_EC; ++e) {
    red[tid * (3 * RS_EC) + e] = mn[e];
    red[tid * (3 * RS_EC) + RS_EC + e] = cs[e];
    red[tid * (3 * RS_EC) + 2 * RS_EC + e] = __int_as_float(cnt[e]);
  }
  __syncthreads();
  for (int item = tid; item < RT * RS_EC; item += 256) {
    const int e = item >> 6, q = item & 63;
    if (e >= a.ne || q >= qrows) continue;
    const int qw = q >> 5, ql = q & 31;
    float m = INFINITY, s = 0.f; int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                  // k = 2 wk + lh
      const int src = ((k >> 1) * 2 + qw) * 64 + (k & 1) * 32 + ql;
      m = fminf(m, red[src * (3 * RS_EC) + e]);
      s += red[src * (3 * RS_EC) + RS_EC + e];
      n += __float_as_int(red[src * (3 * RS_EC) + 2 * RS_EC + e]);
    }
    const int64_t o = ((int64_t)e * RS_MAX_SPLIT + split) * ((int64_t)a.n_tiles * RT) + (int64_t)(d.tile0 + strip) * RT + q;
    a.pmin[o] = m; a.pcs[o] = s; a.pcnt[o] = n;
  }
}

// per (row block, episode of the chunk): the splits of a row in split order, then the block's rows in a fixed order
__global__ __launch_bounds__(256) void rs_rows_kernel(const RsSeq* __restrict__ seq, int n_seq, int n_tiles, int n_rblocks,
                                                      const float* __restrict__ pmin, const float* __restrict__ pcs,
                                                      const int* __restrict__ pcnt, RsBlockPart* __restrict__ bpart) {
  __shared__ float rm[4], rc[4];
  __shared__ long long rn[4];
  const int rb = blockIdx.x, e = blockIdx.y;
  const RsSeq d = seq[rs_find(n_seq, rb, [&](int q) { return seq[q].rb0; })];
  const int t0 = (rb - d.rb0) * (RS_RB_TILES * RT);
  const int64_t plane = (int64_t)n_tiles * RT;
  float smin = 0.f, scs = 0.f; long long scnt = 0;
  for (int i = 0; i < RS_RB_TILES * RT / 256; ++i) {
    const int t = t0 + i * 256 + threadIdx.x;
    if (t >= d.T) break;
    const int64_t o = (int64_t)e * RS_MAX_SPLIT * plane + (int64_t)d.tile0 * RT + t;
    float m = INFINITY, s = 0.f; int n = 0;
    for (int j = 0; j < d.S; ++j) { m = fminf(m, pmin[o + j * plane]); s += pcs[o + j * plane]; n += pcnt[o + j * plane]; }
    smin += m; scs += s; scnt += n;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { smin += __shfl_xor(smin, o); scs += __shfl_xor(scs, o); scnt += __shfl_xor(scnt, o); }
  if ((threadIdx.x & 63) == 0) { rm[threadIdx.x >> 6] = smin; rc[threadIdx.x >> 6] = scs; rn[threadIdx.x >> 6] = scnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    RsBlockPart bp;
    bp.smin = (rm[0] + rm[1]) + (rm[2] + rm[3]); bp.scs = (rc[0] + rc[1]) + (rc[2] + rc[3]); bp.cnt = (rn[0] + rn[1]) + (rn[2] + rn[3]);
    bpart[(int64_t)e * n_rblocks + rb] = bp;
  }
}

// one wave per (video, episode of the chunk): row-block partials (double, lane-strided then a fixed tree), picks by popcount
__global__ __launch_bounds__(64) void rs_join_kernel(const RsSeq* __restrict__ seq, int n_seq, int n_tiles, int n_rblocks,
                                                     const unsigned* __restrict__ bits, const RsBlockPart* __restrict__ bpart, int e0,
                                                     float* __restrict__ reward) {
  const int s = blockIdx.x, e = blockIdx.y, lane = threadIdx.x;
  const RsSeq d = seq[s];
  double smin = 0.0, scs = 0.0; long long far = 0, n = 0;
  for (int b = lane; b < d.nrb; b += 64) {
    const RsBlockPart bp = bpart[(int64_t)e * n_rblocks + d.rb0 + b];
    smin += (double)bp.smin; scs += (double)bp.scs; far += bp.cnt;
  }
  const unsigned* w = bits + ((int64_t)(e0 + e) * n_tiles + d.tile0) * 2;
  for (int i = lane; i < 2 * d.tiles; i += 64) n += __popc(w[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    smin += __shfl_xor(smin, o); scs += __shfl_xor(scs, o); far += __shfl_xor(far, o); n += __shfl_xor(n, o);
  }
  if (lane == 0) {
    float r = 0.f;
    if (n > 0) {
      const double nd = (double)n;
      const double rdiv = n > 1 ? ((double)far + scs) / (nd * (nd - 1.0)) : 0.0;
      const double rrep = exp(-(smin / (double)d.T));
      r = (float)((rdiv + rrep) * 0.5);
    }
    reward[(int64_t)(e0 + e) * n_seq + s] = r;
  }
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_dsn_reward_stream_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t n_episodes) {
  RsWs w;
  if (rs_carve(D, n_seq, seq_off_host, n_episodes, &w) != SUMK_OK) return 0;
  return w.total;
}

extern "C" int32_t sumk_dsn_reward_stream_plan(int32_t n_seq, const int32_t* seq_off_host) {
  if (n_seq <= 0 || !seq_off_host) return 0;
  return rs_plan(n_seq, seq_off_host);
}

extern "C" int sumk_dsn_reward_stream(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                      const float* actions, int32_t n_episodes, int32_t far_sim, int32_t temp_dist_thre,
                                      int32_t col_split, float* reward, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(x && seq_off_dev && actions && reward && workspace, "dsn_reward_stream: null pointer");
  SUMK_ARG(((uintptr_t)x & 15) == 0, "dsn_reward_stream: x must be 16-byte aligned");
  SUMK_ARG(col_split >= 0 && col_split <= RS_MAX_SPLIT, "dsn_reward_stream: col_split=%d (0 = the library's plan, 1..%d)", col_split, RS_MAX_SPLIT);
  RsWs L;
  SUMK_TRY(rs_carve(D, n_seq, seq_off_host, n_episodes, &L));
  if (workspace_bytes < L.total) { set_error("dsn_reward_stream: workspace %zu < required %zu", workspace_bytes, L.total); return SUMK_ERR_WORKSPACE; }
  const int S = col_split ? col_split : rs_plan(n_seq, seq_off_host);
  int64_t blocks = 0;
  for (int s = 0; s < n_seq; ++s) { const int64_t tm = (seq_off_host[s + 1] - seq_off_host[s] + RT - 1) / RT; blocks += tm * std::min<int64_t>(S, tm); }
  SUMK_ARG(blocks < ((int64_t)1 << 31), "dsn_reward_stream: %lld workgroups", (long long)blocks);
  char* ws = (char*)workspace;
  RsSeq* seq = (RsSeq*)(ws + L.seq);
  float* sq = (float*)(ws + L.sq);
  float* rinv = (float*)(ws + L.rinv);
  unsigned* bits = (unsigned*)(ws + L.bits);
  RsBlockPart* bpart = (RsBlockPart*)(ws + L.bpart);
  const int n_tiles = (int)L.tiles, n_rb = (int)L.rblocks;
  const int64_t n_rows = seq_off_host[n_seq];
  prof_begin(SUMK_PROF_REWARD_STREAM_PREP, stream);
  hipLaunchKernelGGL(rs_setup_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, seq_off_dev, n_seq, S, seq);
  const int64_t nw = (int64_t)n_episodes * n_tiles;
  SUMK_ARG((nw + 3) / 4 < ((int64_t)1 << 31), "dsn_reward_stream: %d episodes x %d strips", n_episodes, n_tiles);
  hipLaunchKernelGGL(rs_bits_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, stream, actions, seq, n_seq, n_tiles, n_episodes, n_rows, bits);
  prof_end(SUMK_PROF_REWARD_STREAM_PREP, stream);
  prof_begin(SUMK_PROF_REWARD_STREAM_NORM, stream);
  hipLaunchKernelGGL(rs_norm_kernel, dim3(n_tiles), dim3(256), 0, stream, x, D, seq, n_seq, sq, rinv);
  prof_end(SUMK_PROF_REWARD_STREAM_NORM, stream);
  for (int e0 = 0; e0 < n_episodes; e0 += RS_EC) {
    RsStreamArgs a;
    a.x = x; a.seq = seq; a.bits = bits; a.sq = sq; a.rinv = rinv;
    a.pmin = (float*)(ws + L.pmin); a.pcs = (float*)(ws + L.pcs); a.pcnt = (int*)(ws + L.pcnt);
    a.D = D; a.n_seq = n_seq; a.n_tiles = n_tiles; a.e0 = e0; a.ne = std::min(RS_EC, n_episodes - e0);
    a.far_sim = far_sim; a.thre = temp_dist_thre;
    prof_begin(SUMK_PROF_REWARD_STREAM_PASS, stream);
    hipLaunchKernelGGL(rs_stream_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    prof_end(SUMK_PROF_REWARD_STREAM_PASS, stream);
    prof_begin(SUMK_PROF_REWARD_STREAM_ROWS, stream);
    hipLaunchKernelGGL(rs_rows_kernel, dim3(n_rb, a.ne), dim3(256), 0, stream, seq, n_seq, n_tiles, n_rb, a.pmin, a.pcs, a.pcnt, bpart);
    prof_end(SUMK_PROF_REWARD_STREAM_ROWS, stream);
    prof_begin(SUMK_PROF_REWARD_STREAM_JOIN, stream);
    hipLaunchKernelGGL(rs_join_kernel, dim3(n_seq, a.ne), dim3(64), 0, stream, seq, n_seq, n_tiles, n_rb, bits, bpart, e0, reward);
    prof_end(SUMK_PROF_REWARD_STREAM_JOIN, stream);
  }
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
