// Backward of the streaming multi-head attention in the library's bf16x3 arithmetic: attn_stream_bwd.hip's call on
// v_mfma_f32_32x32x16_bf16, for training on the long videos whose attention is nearly the whole cost of a step.  Opt-in; the fp32
// backward is untouched.  The formulas, the mask index and the NaN rules are those of attn_stream_bwd.hip's header.
//
// Arithmetic (tests/attn_stream_split_bwd_ref.py is its specification): every operand x is hi = bf16(x) (round to nearest even) and
// lo = bf16(x - hi), and each of the seven products is hi.hi + hi.lo + lo.hi with fp32 accumulation, lo.lo dropped:
//   s = q.k;  alpha = exp(fma(s, scale, -m)) * (1 / l) from the statistic the forward saved (v_exp_f32 of t log2(e), as the forward);
//   dA = dctx.v, masked by a select;  dS = alpha (dA~ - delta) scale in fp32;  a~ and dS split IN REGISTERS (a~_hi = bf16(a~),
//   a~_lo = bf16(a~ - a~_hi));  dQ += dS.k, dK += dS^T.q, dV += a~^T.dctx.  delta = dctx . ctx is attn_stream_bwd.hip's fp32 launch.
//
// Launches of one call, all on the caller's stream (it captures into a HIP graph); no cooperative launch, no flag, no atomics:
//   ass_setup_kernel    per-video descriptors (attn_stream_split_common.h)
//   asb_delta_kernel    attn_stream_bwd.hip
//   asb3_split_kernel   Q, K, V, dctx -> bf16 plane pairs in the workspace, once per call; one workgroup per (64-row tile, head, matrix).
//                       ROW-MAJOR planes of all four (A operand of the first products, B operand for the owner strip) and TRANSPOSED
//                       planes of Q, K and dctx (A operand of the accumulating products, which contract over the walked rows), the rows of
//                       a tile in the B operand's order -- both layouts: attn_stream_split_common.h.  28 bytes per (padded row, staged
//                       column).  No conversion of Q, K, V or dctx happens in the tile loops; every padded row and column is written.
//   asb3_dq_kernel      one workgroup (4 waves) per (query strip of 128 rows, head) walks the video's 64-key tiles in ascending order
//   asb3_dkv_kernel     one workgroup per (key strip of 128 rows, head) walks the video's 64-query tiles in ascending order
// Both passes are ONE body (asb3_pass), as in the fp32 unit: an owner strip whose two matrices X1, X2 sit in registers as B fragments of
// both planes, and a walked tile whose matrices Y1, Y2 sit in LDS, row-major for the first products and transposed for the accumulating
// ones.
//   pass   owner X1, X2    walked Y1, Y2    accumulators
//   dQ     Q, dctx         K, V             dQ^T += Y1^T dS^T
//   dK/dV  K, V            Q, dctx          dV^T += Y2^T a~,  dK^T += Y1^T dS
// Lane layout: attn_stream_split.hip's.  First products acc^T = Y (A) x X^T (B): register r of sub-tile sb is owner row li, walked row
// 32 sb + as_crow(r, lh) -- the TRUE walked row, which is where the masks are drawn and the statistics looked up.  Registers 8 s .. 8 s + 7,
// split to bf16, are the B fragment of k-step s of the accumulating product; the transposed planes hold a tile's rows in that order.
//
// Walked rows past T are zeros in the planes and their dS and a~ are set to 0 by a select in the video's last tile, so they contribute
// exactly 0; owner rows past T are the video's last row (clamped) and never stored.  A select, never a multiply, applies the masks.
//
// Staging: every image single-buffered in LDS, the next one in registers HALF an image at a time (NB pieces of 16 bytes per thread): the
// transposed images of tile c travel under the first products of tile c, the row-major images of tile c + 1 under the formation of dS and
// the accumulating products.  Two barriers per tile.  The statistics (m, 1 / l, delta of the tile's 64 queries; dK / dV pass) are
// double-buffered.  LDS per workgroup at dh = 128: dQ pass 100 KiB (K, V row-major 33 KiB each, K transposed 34 KiB), dK / dV pass
// 135.5 KiB (two of each + statistics): one workgroup per CU, one wave per SIMD (__launch_bounds__(256, 1): 512 registers with the AGPRs).
// Registers by count at dh = 128: dQ pass 128 fragments + 64 accumulators + 64 S / dA + 16 staging; dK / dV pass 128 + 128 + 64 + 16.
// Compiler (hipcc -O3, gfx950, CPU-only build) at dh = 128, VGPRs + AGPRs, spilled VGPRs (scratch bytes per lane), without / with dropout:
//   asb3_dq_kernel<4>    256 + 108, none                / 256 + 122, none
//   asb3_dkv_kernel<4>   256 + 206, none                / 256 + 256, 20 (84 B)
// scripts/asm_loop_audit.py: 5 scratch instructions in the tile loop of asb3_dkv_kernel<4, true>, none anywhere else.  The smaller
// instances (NB = 1, 2) take 196 .. 404 registers and do not spill.  scripts/check_waterfalls.sh: 0.
// Measured (scripts/attn_stream_split_train_timing.py, D = 1024, 8 heads, dropout 0.1, T = 8192, per layer): split pass 0.080 ms, delta
// 0.025 ms, dQ pass 1.756 ms (12 T^2 D MFMA FLOP: 0.47 PFLOP/s), dK / dV pass 2.703 ms (16 T^2 D: 0.41 PFLOP/s) -- 4.56 ms against the
// 9.87 ms of the fp32 backward's three launches in the same run.
#include "attn_stream_split_common.h"
#include <algorithm>

namespace sumk {

namespace {

struct Asb3Args {
  // the split pass: the four matrices and where their planes go (tV is unused)
  const float* Q; const float* K; const float* V; const float* G;
  int32_t ldq, ldk, ldv, ldg;
  char* rQ; char* rK; char* rV; char* rG;   // row-major planes
  char* tQ; char* tK; char* tG;             // transposed planes
  // the passes
  const char* X1; const char* X2;           // owner strip, row-major planes: dQ pass Q, dctx; dK / dV pass K, V
  const char* Y1; const char* Y2;           // walked tiles, row-major planes:  dQ pass K, V;   dK / dV pass Q, dctx
  const char* Y1t; const char* Y2t;         // walked tiles, transposed planes: dQ pass K, -;   dK / dV pass Q, dctx
  float* O1; float* O2;                     // dQ pass: dQ, unused; dK / dV pass: dK, dV
  int32_t ldo1, ldo2;
  const float2* ml; const float* delta; const AssSeq* seq;
  int64_t RP;                               // padded rows of the batch (a multiple of 64)
  int32_t dh, heads, n_seq; float scale;
  uint64_t seed; uint32_t site, thr; float keep_scale;
};

// One workgroup per (64-row tile of a video, head, matrix z = Q, K, V, dctx): the tile's rows as [hi DP | lo DP], and (not V)
// transposed through LDS.
template <int NB>
__global__ __launch_bounds__(256) void asb3_split_kernel(Asb3Args a) {
  constexpr int DP = 32 * NB, G8 = DP / 8, C4 = DP / 4;
  __shared__ __attribute__((aligned(16))) unsigned short vt[DP * 128];   // [d][hi 64 | lo 64]
  const int tid = threadIdx.x, h = blockIdx.y, z = blockIdx.z, dh = a.dh;
  const float* X = z == 0 ? a.Q : z == 1 ? a.K : z == 2 ? a.V : a.G;
  const int ld = z == 0 ? a.ldq : z == 1 ? a.ldk : z == 2 ? a.ldv : a.ldg;
  char* R = z == 0 ? a.rQ : z == 1 ? a.rK : z == 2 ? a.rV : a.rG;
  char* Tp = z == 0 ? a.tQ : z == 1 ? a.tK : z == 2 ? nullptr : a.tG;
  const int64_t ptile = blockIdx.x;                                      // tile among the batch's padded tiles
  const AssSeq d = ass_find(a.seq, a.n_seq, ptile * AS_KT, false);
  const int k0 = (int)(ptile * AS_KT - d.prow0);                         // the tile's first row inside the video
  const int64_t hcol = (int64_t)h * dh;
  for (int idx = tid; idx < AS_KT * G8; idx += 256) {                    // row-major: 8 columns per item
    const int r = idx / G8, c8 = (idx % G8) * 8;
    const int64_t src = d.row0 + k0 + r, dst = (((int64_t)h * a.RP + ptile * AS_KT + r) * (2 * DP) + c8) * 2;
    f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
    if (k0 + r < d.T && c8 < dh) { x0 = *reinterpret_cast<const f32x4*>(X + src * ld + hcol + c8); x1 = *reinterpret_cast<const f32x4*>(X + src * ld + hcol + c8 + 4); }
    u32x2 p0[2], p1[2];
    split4<2>(x0, p0); split4<2>(x1, p1);
    const u32x4 hi = {p0[0][0], p0[0][1], p1[0][0], p1[0][1]}, lo = {p0[1][0], p0[1][1], p1[1][0], p1[1][1]};
    *reinterpret_cast<u32x4*>(R + dst) = hi;
    *reinterpret_cast<u32x4*>(R + dst + 2 * DP) = lo;
  }
  if (!Tp) return;                                                       // workgroup-uniform
  // transposed: row on the lane (the LDS writes of a wave are 64 consecutive positions of one image row), 4 columns per item
  for (int idx = tid; idx < AS_KT * C4; idx += 256) {
    const int r = idx % AS_KT, c4 = (idx / AS_KT) * 4;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (k0 + r < d.T && c4 < dh) x = *reinterpret_cast<const f32x4*>(X + (d.row0 + k0 + r) * ld + hcol + c4);
    u32x2 p[2];
    split4<2>(x, p);
    const int pos = ass_perm(r);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vt[(c4 + i) * 128 + pos] = (unsigned short)(p[0][i >> 1] >> (16 * (i & 1)));
      vt[(c4 + i) * 128 + 64 + pos] = (unsigned short)(p[1][i >> 1] >> (16 * (i & 1)));
    }
  }
  __syncthreads();
  char* tdst = Tp + ((int64_t)h * (a.RP / AS_KT) + ptile) * (DP * 256);
  for (int idx = tid; idx < DP * 16; idx += 256)
    *reinterpret_cast<u32x4*>(tdst + (int64_t)idx * 16) = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(vt) + idx * 16);
}

template <int NB, bool DKV> struct Asb3Geom {
  static constexpr int DP = 32 * NB, KS = DP / 16;            // staged columns; k-steps of a first product
  static constexpr int RPITCH = 4 * DP + 16;                  // bytes of a row-major image row: [hi DP | lo DP] + 16
  static constexpr int RIMG = AS_KT * RPITCH, TIMG = DP * ASS_VP;
  static constexpr int NT = DKV ? 2 : 1;                      // transposed images
  static constexpr int SST = 2 * RIMG + NT * TIMG;            // byte offset of the statistics (dK / dV pass: 2 buffers x 3 x 64 floats)
  static constexpr int LDS = SST + (DKV ? 2 * 3 * AS_KT * 4 : 0);
};

template <int NB, bool DKV, bool DROP>
__device__ __forceinline__ void asb3_pass(const Asb3Args& a, char* lds) {
  using G = Asb3Geom<NB, DKV>;
  constexpr int DP = G::DP, KS = G::KS, KP = G::RPITCH, NST = NB;   // NST: 16-byte pieces per thread and half image (8 DP / 256)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int sg = blockIdx.x / a.heads, h = blockIdx.x % a.heads, dh = a.dh;
  const AssSeq d = ass_find(a.seq, a.n_seq, sg, true);
  const int T = d.T;
  const int r0 = (sg - d.strip0) * AS_QS + wave * 32;
  const bool live = r0 < T;                                         // wave-uniform: a wave past the video only stages
  const int orow = min(r0 + li, T - 1);                             // clamped: such rows are never stored

  // owner fragments of both planes of both matrices: k-step g, element j -> X[owner row][16 g + 8 lh + j]
  bf16x8 x1h[KS], x1l[KS], x2h[KS], x2l[KS];
  {
    const int64_t at = (((int64_t)h * a.RP + d.prow0 + orow) * (2 * DP) + 8 * lh) * 2;
    const char* p1 = a.X1 + at;
    const char* p2 = a.X2 + at;
#pragma unroll
    for (int g = 0; g < KS; ++g) {
      x1h[g] = ass_ld(p1 + 32 * g); x1l[g] = ass_ld(p1 + 32 * g + 2 * DP);
      x2h[g] = ass_ld(p2 + 32 * g); x2l[g] = ass_ld(p2 + 32 * g + 2 * DP);
    }
  }
  // dQ pass: the statistic and delta of the lane's own query row
  float om = 0.f, oil = 0.f, odl = 0.f;
  if (!DKV) {
    const int64_t si = (d.row0 + orow) * (int64_t)a.heads + h;
    const float2 t = a.ml[si];
    om = t.x; oil = 1.0f / t.y; odl = a.delta[si];
  }

  const int64_t rbase = ((int64_t)h * a.RP + d.prow0) * (4 * DP);                      // tile c: + c * 256 DP bytes, contiguous
  const int64_t tbase = ((int64_t)h * (a.RP / AS_KT) + d.prow0 / AS_KT) * (DP * 256);
  const char* Y1r = a.Y1 + rbase;
  const char* Y2r = a.Y2 + rbase;
  const char* Y1t = a.Y1t + tbase;
  const char* Y2t = DKV ? a.Y2t + tbase : nullptr;

  // staging of HALF an image (128 DP bytes): thread -> NST pieces of 16 bytes, piece idx = 256 NB half + tid + 256 i of the tile
  u32x4 st[NST];
  auto gload = [&](const char* base, int c, int half) {
    const char* p = base + (int64_t)c * (DP * 256) + (256 * NB * half + tid) * 16;
#pragma unroll
    for (int i = 0; i < NST; ++i) st[i] = *reinterpret_cast<const u32x4*>(p + 4096 * i);
  };
  auto rwrite = [&](char* img, int half) {        // a row-major row is DP / 4 pieces
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = 256 * NB * half + tid + 256 * i;
      *reinterpret_cast<u32x4*>(img + (idx / (DP / 4)) * KP + (idx % (DP / 4)) * 16) = st[i];
    }
  };
  auto twrite = [&](char* img, int half) {        // a transposed row is 16 pieces
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = 256 * NB * half + tid + 256 * i;
      *reinterpret_cast<u32x4*>(img + (idx >> 4) * ASS_VP + (idx & 15) * 16) = st[i];
    }
  };
  // dK / dV pass: m, 1 / l, delta of the tile's 64 queries (they vary per accumulator register, not per lane); rows past T: zeros
  float* sst = reinterpret_cast<float*>(lds + G::SST);
  float stm = 0.f, stil = 0.f, stdl = 0.f;
  auto sload = [&](int c) {
    if (DKV && tid < AS_KT) {
      const int wr = c * AS_KT + tid;
      stm = 0.f; stil = 0.f; stdl = 0.f;
      if (wr < T) {
        const int64_t si = (d.row0 + wr) * (int64_t)a.heads + h;
        const float2 t = a.ml[si];
        stm = t.x; stil = 1.0f / t.y; stdl = a.delta[si];
      }
    }
  };
  auto swrite = [&](int c) {
    if (DKV && tid < AS_KT) { float* b = sst + (c & 1) * (3 * AS_KT); b[tid] = stm; b[AS_KT + tid] = stil; b[2 * AS_KT + tid] = stdl; }
  };

  char* R1 = lds;
  char* R2 = lds + G::RIMG;
  char* T1 = lds + 2 * G::RIMG;
  char* T2 = lds + 2 * G::RIMG + G::TIMG;         // dK / dV pass only
  const char* rfrag1 = R1 + li * KP + 16 * lh;    // + 32 sb KP + 32 g [+ 2 DP: lo]
  const char* rfrag2 = R2 + li * KP + 16 * lh;
  const char* tfrag1 = T1 + li * ASS_VP + 16 * lh;   // + 32 b VP + 64 sb + 32 s [+ 128: lo]
  const char* tfrag2 = T2 + li * ASS_VP + 16 * lh;
  const int nt = (T + AS_KT - 1) / AS_KT;
  f32x16 o1[NB], o2[DKV ? NB : 1], s0, s1, da0, da1;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) o1[b][r] = 0.f;
#pragma unroll
  for (int b = 0; b < (DKV ? NB : 1); ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) o2[b][r] = 0.f;
  constexpr float LOG2E = 1.4426950408889634f;

  // first product over the k-steps [g0, g1): acc^T += image (A) x owner fragments (B), three MFMAs per step and sub-tile
  auto first = [&](const char* rfrag, const bf16x8 (&xh)[KS], const bf16x8 (&xl)[KS], f32x16& acc0, f32x16& acc1, int g0, int g1) {
#pragma unroll
    for (int g = g0; g < g1; ++g) {
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        f32x16& acc = sb ? acc1 : acc0;
        const bf16x8 yh = ass_ld(rfrag + 32 * sb * KP + 32 * g), yl = ass_ld(rfrag + 32 * sb * KP + 32 * g + 2 * DP);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xh[g], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xl[g], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yl, xh[g], acc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);          // keep the compiler from hoisting every step's reads (register budget)
    }
  };
  // accumulating product of sub-tile sb: the weights split in registers, then 2 k-steps x NB blocks x 3 MFMAs
  auto accum = [&](const char* tfrag, const f32x16& w, int sb, f32x16* out) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f32x8 p;
#pragma unroll
      for (int j = 0; j < 8; ++j) p[j] = w[8 * s + j];
      const bf16x8 ph = __builtin_convertvector(p, bf16x8);
      const bf16x8 pl = __builtin_convertvector(p - __builtin_convertvector(ph, f32x8), bf16x8);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const bf16x8 yh = ass_ld(tfrag + 32 * b * ASS_VP + 64 * sb + 32 * s), yl = ass_ld(tfrag + 32 * b * ASS_VP + 64 * sb + 32 * s + 128);
        out[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, ph, out[b], 0, 0, 0);
        out[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yl, ph, out[b], 0, 0, 0);
        out[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, pl, out[b], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  gload(Y1r, 0, 0); rwrite(R1, 0);
  gload(Y1r, 0, 1); rwrite(R1, 1);
  gload(Y2r, 0, 0); rwrite(R2, 0);
  gload(Y2r, 0, 1); rwrite(R2, 1);
  sload(0); swrite(0);
  for (int c = 0; c < nt; ++c) {
    const bool more = c + 1 < nt;
    __syncthreads();                              // the row-major images (and statistics) of tile c are visible; every wave is done
                                                  // with the transposed images of tile c - 1
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; da0[r] = 0.f; da1[r] = 0.f; }
    gload(Y1t, c, 0);                             // the transposed images travel under the first products, half an image at a time
    if (live) first(rfrag1, x1h, x1l, s0, s1, 0, KS / 2);
    twrite(T1, 0);
    gload(Y1t, c, 1);
    if (live) first(rfrag1, x1h, x1l, s0, s1, KS / 2, KS);
    twrite(T1, 1);
    if (DKV) {
      gload(Y2t, c, 0);
      if (live) first(rfrag2, x2h, x2l, da0, da1, 0, KS / 2);
      twrite(T2, 0);
      gload(Y2t, c, 1);
      if (live) first(rfrag2, x2h, x2l, da0, da1, KS / 2, KS);
      twrite(T2, 1);
    } else if (live) first(rfrag2, x2h, x2l, da0, da1, 0, KS);
    __syncthreads();                              // the transposed images of tile c are visible; every wave is done with the row-major ones
    if (more) { gload(Y1r, c + 1, 0); sload(c + 1); }   // the row-major images of tile c + 1 travel under dS and the accumulating products
    if (live) {
      const bool partial = (c + 1) * AS_KT > T;   // the video's last tile: walked rows past T contribute exactly 0
      const float* sb_ = sst + (c & 1) * (3 * AS_KT);
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          f32x16& sv = sb ? s1 : s0;
          f32x16& dv = sb ? da1 : da0;
          const int tr = 32 * sb + as_crow(r, lh), wr = c * AS_KT + tr;     // walked row: inside the tile, inside the video (TRUE row)
          float m = om, il = oil, dl = odl;
          if (DKV) { m = sb_[tr]; il = sb_[AS_KT + tr]; dl = sb_[2 * AS_KT + tr]; }
          const float alpha = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[r], a.scale, -m) * LOG2E) * il;
          float dA = dv[r], at = alpha;
          if (DROP) {
            const uint64_t idx = DKV ? as_drop_idx(d.row0 + wr, a.heads, h, r0 + li) : as_drop_idx(d.row0 + orow, a.heads, h, wr);
            const bool keep = dropout_keep(a.seed, a.site, idx, a.thr);
            dA = keep ? dA * a.keep_scale : 0.f;
            at = keep ? alpha * a.keep_scale : 0.f;
          }
          float ds = alpha * (dA - dl) * a.scale;
          if (partial && wr >= T) { ds = 0.f; at = 0.f; }
          dv[r] = ds; sv[r] = at;
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (more) { rwrite(R1, 0); swrite(c + 1); gload(Y1r, c + 1, 1); }
    if (live) { if (DKV) accum(tfrag2, s0, 0, o2); else accum(tfrag1, da0, 0, o1); }
    if (more) { rwrite(R1, 1); gload(Y2r, c + 1, 0); }
    if (live) { if (DKV) accum(tfrag2, s1, 1, o2); else accum(tfrag1, da1, 1, o1); }
    if (more) { rwrite(R2, 0); gload(Y2r, c + 1, 1); }
    if (DKV && live) accum(tfrag1, da0, 0, o1);
    if (more) rwrite(R2, 1);
    if (DKV && live) accum(tfrag1, da1, 1, o1);
  }

  const int q = r0 + li;
  if (!live || q >= T) return;
  // block b register r: out[owner row][d = 32 b + as_crow(r, lh)]: four consecutive columns per register quad (dh % 8 == 0 keeps it whole)
  auto store = [&](float* O, int ld, const f32x16* o) {
    float* p = O + (d.row0 + q) * (int64_t)ld + (int64_t)h * dh;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int dd = 32 * b + 8 * r4 + 4 * lh;
        if (dd < dh) *reinterpret_cast<float4*>(p + dd) = make_float4(o[b][4 * r4], o[b][4 * r4 + 1], o[b][4 * r4 + 2], o[b][4 * r4 + 3]);
      }
  };
  store(a.O1, a.ldo1, o1);
  if constexpr (DKV) store(a.O2, a.ldo2, o2);
}

template <int NB, bool DROP>
__global__ __launch_bounds__(256, 1) void asb3_dq_kernel(Asb3Args a) {
  extern __shared__ __attribute__((aligned(16))) char asb3_lds[];
  asb3_pass<NB, false, DROP>(a, asb3_lds);
}
template <int NB, bool DROP>
__global__ __launch_bounds__(256, 1) void asb3_dkv_kernel(Asb3Args a) {
  extern __shared__ __attribute__((aligned(16))) char asb3_lds[];
  asb3_pass<NB, true, DROP>(a, asb3_lds);
}

struct Asb3Layout { size_t desc, delta, r[4], t[3], total; int64_t RP, strips; int nb; };

int asb3_layout(const char* who, int D, int heads, int n_seq, const int32_t* off, int precision, Asb3Layout* L) {
  SUMK_TRY(ass_check(who, D, heads, n_seq, off, precision, &L->RP, &L->strips, &L->nb));
  const size_t plane = (size_t)heads * (size_t)L->RP * (size_t)(32 * L->nb) * 4;   // hi + lo, 2 bytes each
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  L->desc = take((size_t)n_seq * sizeof(AssSeq));
  L->delta = take((size_t)off[n_seq] * (size_t)heads * sizeof(float));
  for (int i = 0; i < 4; ++i) L->r[i] = take(plane);
  for (int i = 0; i < 3; ++i) L->t[i] = take(plane);
  L->total = p;
  return SUMK_OK;
}

template <int NB>
int asb3_launch(Asb3Args& a, const Asb3Layout& L, hipStream_t stream) {
  prof_begin(SUMK_PROF_ATTN_STREAM_SPLIT_BWD_PLANES, stream);
  hipLaunchKernelGGL(asb3_split_kernel<NB>, dim3((unsigned)(L.RP / AS_KT), (unsigned)a.heads, 4), dim3(256), 0, stream, a);
  prof_end(SUMK_PROF_ATTN_STREAM_SPLIT_BWD_PLANES, stream);
  const unsigned blocks = (unsigned)(L.strips * a.heads);
  const bool drop = a.thr != 0;
  a.X1 = a.rQ; a.X2 = a.rG; a.Y1 = a.rK; a.Y2 = a.rV; a.Y1t = a.tK; a.Y2t = nullptr;
  prof_begin(SUMK_PROF_ATTN_STREAM_SPLIT_BWD_DQ, stream);
  const int rc = drop ? as_launch<asb3_dq_kernel<NB, true>>(a, blocks, Asb3Geom<NB, false>::LDS, stream)
                      : as_launch<asb3_dq_kernel<NB, false>>(a, blocks, Asb3Geom<NB, false>::LDS, stream);
  prof_end(SUMK_PROF_ATTN_STREAM_SPLIT_BWD_DQ, stream);
  return rc;
}

template <int NB>
int asb3_launch_dkv(Asb3Args& a, const Asb3Layout& L, hipStream_t stream) {
  const unsigned blocks = (unsigned)(L.strips * a.heads);
  a.X1 = a.rK; a.X2 = a.rV; a.Y1 = a.rQ; a.Y2 = a.rG; a.Y1t = a.tQ; a.Y2t = a.tG;
  prof_begin(SUMK_PROF_ATTN_STREAM_SPLIT_BWD_DKV, stream);
  const int rc = a.thr != 0 ? as_launch<asb3_dkv_kernel<NB, true>>(a, blocks, Asb3Geom<NB, true>::LDS, stream)
                            : as_launch<asb3_dkv_kernel<NB, false>>(a, blocks, Asb3Geom<NB, true>::LDS, stream);
  prof_end(SUMK_PROF_ATTN_STREAM_SPLIT_BWD_DKV, stream);
  return rc;
}

}  // namespace

size_t attn_stream_split_bwd_ws_bytes(int D, int heads, int n_seq, const int32_t* off, int precision) {
  Asb3Layout L;
  return asb3_layout("attn_stream_split_backward", D, heads, n_seq, off, precision, &L) == SUMK_OK ? L.total : 0;
}

int launch_attn_stream_split_bwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* ctx, int ldc,
                                 const float* dctx, int ldd, const float* stats, int D, int heads, int n_seq, const int32_t* off_host,
                                 const int32_t* off_dev, float scale, int precision, Drop dl, uint32_t site, float* dQ, int lddq, float* dK,
                                 int lddk, float* dV, int lddv, void* ws, hipStream_t stream) {
  const char* who = "attn_stream_split_backward";
  SUMK_ARG(Q && K && V && ctx && dctx && stats && dQ && dK && dV && off_dev && ws, "%s: null pointer", who);
  Asb3Layout L;
  SUMK_TRY(asb3_layout(who, D, heads, n_seq, off_host, precision, &L));
  SUMK_ARG(heads <= 65535, "%s: n_heads=%d", who, heads);
  const int lds[8] = {ldq, ldk, ldv, ldc, ldd, lddq, lddk, lddv};
  for (int i = 0; i < 8; ++i) {
    SUMK_ARG(lds[i] >= D, "%s: leading dimension %d (argument %d of 8) must be at least D=%d", who, lds[i], i, D);
    SUMK_ARG(lds[i] % 4 == 0, "%s: leading dimension %d (argument %d of 8) must be a multiple of 4", who, lds[i], i);
  }
  SUMK_ARG(((uintptr_t)stats & 7) == 0, "%s: stats must be 8-byte aligned", who);
  SUMK_TRY(as_check_operands(who, (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)ctx | (uintptr_t)dctx | (uintptr_t)dQ | (uintptr_t)dK | (uintptr_t)dV | (uintptr_t)ws,
                             "Q, K, V, ctx, dctx, dQ, dK, dV and the workspace", scale));
  SUMK_ARG(!dl.seed_dev, "%s: no device seed word", who);
  char* w = (char*)ws;
  float* delta = (float*)(w + L.delta);
  hipLaunchKernelGGL(ass_setup_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, off_dev, n_seq, (AssSeq*)(w + L.desc));
  launch_attn_stream_bwd_delta(ctx, ldc, dctx, ldd, delta, off_host[n_seq], heads, D / heads, stream);
  Asb3Args a;
  a.Q = Q; a.K = K; a.V = V; a.G = dctx; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldg = ldd;
  a.rQ = w + L.r[0]; a.rK = w + L.r[1]; a.rV = w + L.r[2]; a.rG = w + L.r[3];
  a.tQ = w + L.t[0]; a.tK = w + L.t[1]; a.tG = w + L.t[2];
  a.X1 = a.X2 = a.Y1 = a.Y2 = a.Y1t = a.Y2t = nullptr;
  a.ml = (const float2*)stats; a.delta = delta; a.seq = (const AssSeq*)(w + L.desc); a.RP = L.RP;
  a.dh = D / heads; a.heads = heads; a.n_seq = n_seq; a.scale = scale;
  a.seed = dl.seed; a.site = site; a.thr = dl.thr; a.keep_scale = dl.scale;
  a.O1 = dQ; a.ldo1 = lddq; a.O2 = nullptr; a.ldo2 = 0;
  SUMK_TRY(L.nb == 1 ? asb3_launch<1>(a, L, stream) : L.nb == 2 ? asb3_launch<2>(a, L, stream) : asb3_launch<4>(a, L, stream));
  a.O1 = dK; a.ldo1 = lddk; a.O2 = dV; a.ldo2 = lddv;
  SUMK_TRY(L.nb == 1 ? asb3_launch_dkv<1>(a, L, stream) : L.nb == 2 ? asb3_launch_dkv<2>(a, L, stream) : asb3_launch_dkv<4>(a, L, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_attn_stream_split_backward_workspace_bytes(int32_t D, int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host,
                                                                  int32_t precision) {
  return attn_stream_split_bwd_ws_bytes(D, n_heads, n_seq, seq_off_host, precision);
}

extern "C" int sumk_attn_stream_split_backward(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv,
                                               const float* ctx, int32_t ldc, const float* dctx, int32_t ldd, const float* stats, int32_t D,
                                               int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                               float scale, float dropout_p, uint64_t seed, uint32_t site, float* dQ, int32_t lddq, float* dK,
                                               int32_t lddk, float* dV, int32_t lddv, void* workspace, size_t workspace_bytes, void* stream,
                                               int32_t precision) {
  const char* who = "attn_stream_split_backward";
  SUMK_ARG(workspace, "%s: null pointer", who);
  SUMK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p=%g must lie in [0, 1)", who, (double)dropout_p);
  Asb3Layout L;
  SUMK_TRY(asb3_layout(who, D, n_heads, n_seq, seq_off_host, precision, &L));
  if (workspace_bytes < L.total) { set_error("%s: workspace %zu < required %zu", who, workspace_bytes, L.total); return SUMK_ERR_WORKSPACE; }
  return launch_attn_stream_split_bwd(Q, ldq, K, ldk, V, ldv, ctx, ldc, dctx, ldd, stats, D, n_heads, n_seq, seq_off_host, seq_off_dev, scale,
                                      precision, make_drop(dropout_p, seed), site, dQ, lddq, dK, lddk, dV, lddv, workspace,
                                      (hipStream_t)stream);
}
