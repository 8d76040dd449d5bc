// Streaming multi-head attention in the library's bf16x3 arithmetic: attn_stream.hip's call on v_mfma_f32_32x32x16_bf16, for the long
// videos whose attention is nearly the whole cost of a scoring call.  Scoring and the training forward, opt-in; the fp32 kernel is untouched.
//
//   ctx[rows of v, h dh : (h + 1) dh] = softmax_j(scale Q_h K_h^T) V_h          per video v and head h of a packed batch, no mask
//
// Arithmetic (tests/attn_stream_split_ref.py is its specification): every operand x is hi = bf16(x) (round to nearest even) and
// lo = bf16(x - hi) -- split4<2> of pw_common.h -- and a product is hi.hi + hi.lo + lo.hi with fp32 accumulation, lo.lo dropped:
//   s = q_hi.k_hi + q_hi.k_lo + q_lo.k_hi;  online softmax in fp32 exactly as as_stream_kernel (m' = max(m, scale max s), p =
//   exp(fma(s, scale, -m')), rescale on every tile, no threshold, no data-dependent branch; l takes the fp32 p);  the weights split in
//   registers, p_hi = bf16(p), p_lo = bf16(p - p_hi);  O += p_hi.v_hi + p_hi.v_lo + p_lo.v_hi;  ctx = O / l, lse = m + log(l).
// The exponential is v_exp_f32 of t log2(e) with t = fma(s, scale, -m') the specification's argument: t is rounded once as there, the
// extra product moves p by |t| 2^-24 relative (nothing for the weights that matter) and v_exp_f32 is good to 1 ulp -- against 2^-16 per
// product of the arithmetic around it.  The accurate expf costs about 15 instructions per weight, which after the MFMA time fell by 5x
// would be longer than the MFMAs.
//
// Launches of one call, all on the caller's stream (it captures into a HIP graph); no cooperative launch, no flag, no atomics:
//   ass_setup_kernel   per-video descriptors: first row, first PADDED row (videos are padded to whole 64-key tiles in the planes), frames,
//                      first query strip
//   ass_split_kernel   Q, K, V -> bf16 plane pairs in the workspace, 4 bytes per staged element; one workgroup per (64-row tile, head).
//                      No conversion of Q, K or V happens in the tile loop.  Every padded row and column is written (zeros), so the
//                      call does not depend on what the workspace held.
//                        Q, K   [head][padded row][hi DP | lo DP]: a 64-key K tile is ONE contiguous block of 256 DP bytes
//                        V      [head][tile][d][hi 64 keys | lo 64 keys], TRANSPOSED, the keys of a tile in the order the second
//                               product's B operand has them (below): position p holds key p with bits 2 and 3 swapped
//   ass_kernel         one workgroup (4 waves) per (query strip of 128 rows, head), block = strip * heads + head as in attn_stream.hip;
//                      a wave owns 32 whole query rows, the workgroup walks the video's 64-key tiles in ascending order.
//
// Lane layout (lane = (li = lane & 31, lh = lane >> 5); v_mfma_f32_32x32x16_bf16 everywhere):
//   First product  S^T = K_tile (A) x Q^T (B): A[key li][k = 8 lh + j] = K[32 sb + li][16 g + 8 lh + j], one ds_read_b128 per plane of
//     the K image; B[k][query li] = Q[query li][16 g + 8 lh + j], the Q fragments of both planes in registers for the whole walk.
//     Accumulator register r of sub-tile sb: query li, key 32 sb + as_crow(r, lh).
//   Second product  O^T += V^T (A) x P^T (B): registers 8 s .. 8 s + 7 of that accumulator, converted pairwise to bf16, ARE the B
//     fragment of k-step s: element j of lane half lh is key 16 s + 8 (j >> 2) + 4 lh + (j & 3).  The A fragment must use the same
//     order; the split pass stored V^T that way, so it is one ds_read_b128 per plane at [d = 32 b + li][32 sb + 16 s + 8 lh].  P is
//     never stored and never changes lane.  Block b register r: O[query li][d = 32 b + as_crow(r, lh)]: the rescale is a per-lane multiply,
//     the store four consecutive columns per register quad.
// Keys past T get the logit -inf (p = 0 exactly; their V columns are zeros in the planes), padded head columns add fma(0, 0, acc).
//
// Staging: K and V tiles single-buffered in LDS (K image 64 x (4 DP + 16) bytes, V image DP x 272 bytes: pitches = 4 dwords mod 32,
// conflict-free for the b128 reads), the next tile in registers half a tile at a time as in attn_stream.hip: V(c) under the first
// product, K(c + 1) under the softmax and the second product.  Two barriers per tile.
//
// Instances by staged width DP = 32 NB (dh = 40 or 104 run the next wider one on zero columns); dh % 8 == 0, dh <= 128.
//   NB  LDS per workgroup   MFMAs per tile and wave   registers per lane by count                             as the compiler allots (CPU-only build)
//   1   17 KiB              12 + 12                   Q 16 + O 16 + S 32 + staging 4 + fragments 32 = 100     109 VGPRs, no spill
//   2   34 KiB              24 + 24                   Q 32 + O 32 + S 32 + staging 8 + fragments 32 = 136     146 VGPRs, no spill
//   4   67 KiB (2 per CU)   48 + 48                   Q 64 + O 64 + S 32 + staging 16 + fragments 32 = 208    231 of 256 VGPRs, no spill: 2 waves per SIMD
// (fragments: 2 planes of P for one k-step, K or V fragments of both planes one step ahead, addresses.)  No AGPRs, no scratch in any
// instance; scripts/check_waterfalls.sh: 0.
// Vector-ALU work per tile and lane beside them, by count: 32 fmax + exchange, 32 fma + 32 mul + 32 v_exp + 32 adds, the P split (16 cvt_pk,
// 32 unpack shifts, 32 subtractions, 16 cvt_pk), 16 NB multiplies of O, the staging addresses.  As compiled the tile loop holds 441 / 458 /
// 498 vector-ALU instructions (NB = 1 / 2 / 4; 33 v_exp_f32; about 100 of them are the -inf mask of a video's partial last tile, skipped
// on every other tile) beside its 24 / 48 / 96 MFMAs of 8 passes, 21 / 41 / 81 LDS and 4 / 8 / 16 global instructions: at dh = 128 the
// vector work (about 400 x 4 cycles) is half of the MFMA time (96 x 32 cycles) where in the fp32 kernel it was 17 %.
// Measured (scripts/attn_stream_split_timing.py, D = 1024, 8 heads, split pass + attention per layer): 0.750 ms at T = 8192 against
// 2.239 ms of the fp32 launch (2.99x), 44.3 ms against 136.2 ms at T = 65 536 (3.08x); the attention launch alone runs its 12 T^2 D FLOP at
// 1.17 / 1.20 PFLOP/s, the split pass takes 0.044 / 0.339 ms.
//
// The training form (sumk_attn_stream_split_train; its backward: attn_stream_split_bwd.hip) is the same kernel with the two additions of
// as_stream_kernel<NB, DROP>.  The statistic (m, l) per (row, head) is written whenever a.ml is given.  DROP instances drop the weights:
// the running sum l takes the undropped p, the second product keep ? p / (1 - p) : 0 with the dense path's mask index at the TRUE key of
// each accumulator register (32 sb + as_crow(r, lh); only the planes are permuted).  With dropout_p == 0 the non-DROP instances run: no hash
// in the instruction stream, ctx has the bits of sumk_attn_stream_split.  The hash costs registers: ass_kernel<4, true> takes all 256 VGPRs
// of its two-waves-per-SIMD budget and spills 83 (336 B of scratch), as the fp32 twin does (85); NB = 1, 2 take 218 / 255, no spill.
// Measured (scripts/attn_stream_split_train_timing.py, D = 1024, 8 heads, dropout 0.1): 1.486 ms at T = 8192 against 2.800 ms of the fp32
// training forward in the same run.
#include "attn_stream_split_common.h"
#include <algorithm>

namespace sumk {

namespace {
struct AssArgs {
  const float* Q; const float* K; const float* V; float* ctx; float* lse; const AssSeq* seq;
  char* qp; char* kp; char* vp;                 // the planes
  int64_t RP;                                   // padded rows of the batch (a multiple of 64)
  int32_t ldq, ldk, ldv, ldc, dh, heads, n_seq; float scale;
  // the training form: the statistic (m, l) per (row, head) for the backward, and the dropout of the weights (DROP instances only)
  float2* ml; uint64_t seed; uint32_t site, thr; float keep_scale;
};

// One workgroup per (64-row tile of a video, head): the tile's rows of Q and K as [hi DP | lo DP], of V transposed through LDS.
template <int NB>
__global__ __launch_bounds__(256) void ass_split_kernel(AssArgs a) {
  constexpr int DP = 32 * NB, G8 = DP / 8, C4 = DP / 4;
  __shared__ __attribute__((aligned(16))) unsigned short vt[DP * 128];   // [d][hi 64 | lo 64]
  const int tid = threadIdx.x, h = blockIdx.y, dh = a.dh;
  const int64_t ptile = blockIdx.x;                                      // tile among the batch's padded tiles
  const AssSeq d = ass_find(a.seq, a.n_seq, ptile * AS_KT, false);
  const int k0 = (int)(ptile * AS_KT - d.prow0);                         // the tile's first row inside the video
  const int64_t hcol = (int64_t)h * dh;
  // Q and K: 8 columns per item
  for (int idx = tid; idx < AS_KT * G8; idx += 256) {
    const int r = idx / G8, c8 = (idx % G8) * 8;
    const bool ok = k0 + r < d.T && c8 < dh;
    const int64_t src = (d.row0 + k0 + r), dst = (((int64_t)h * a.RP + ptile * AS_KT + r) * (2 * DP) + c8) * 2;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const float* X = w ? a.K : a.Q;
      const int ld = w ? a.ldk : a.ldq;
      char* P = w ? a.kp : a.qp;
      f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
      if (ok) { x0 = *reinterpret_cast<const f32x4*>(X + src * ld + hcol + c8); x1 = *reinterpret_cast<const f32x4*>(X + src * ld + hcol + c8 + 4); }
      u32x2 p0[2], p1[2];
      split4<2>(x0, p0); split4<2>(x1, p1);
      const u32x4 hi = {p0[0][0], p0[0][1], p1[0][0], p1[0][1]}, lo = {p0[1][0], p0[1][1], p1[1][0], p1[1][1]};
      *reinterpret_cast<u32x4*>(P + dst) = hi;
      *reinterpret_cast<u32x4*>(P + dst + 2 * DP) = lo;
    }
  }
  // V: key on the lane (the LDS writes of a wave are 64 consecutive positions of one row), 4 columns per item
  for (int idx = tid; idx < AS_KT * C4; idx += 256) {
    const int r = idx % AS_KT, c4 = (idx / AS_KT) * 4;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (k0 + r < d.T && c4 < dh) x = *reinterpret_cast<const f32x4*>(a.V + (d.row0 + k0 + r) * a.ldv + hcol + c4);
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
  char* vdst = a.vp + ((int64_t)h * (a.RP / AS_KT) + ptile) * (DP * 256);
  for (int idx = tid; idx < DP * 16; idx += 256)
    *reinterpret_cast<u32x4*>(vdst + (int64_t)idx * 16) = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(vt) + idx * 16);
}

template <int NB> struct AssGeom {
  static constexpr int DP = 32 * NB, KS = DP / 16;            // staged columns; k-steps of the first product
  static constexpr int KP = 4 * DP + 16;                      // bytes of a K image row: [hi DP | lo DP] + 16
  static constexpr int KIMG = AS_KT * KP, VIMG = DP * ASS_VP; // bytes of the images
  static constexpr int LDS = KIMG + VIMG;
};

// DROP: the training form with dropout of the weights -- the running sum takes the undropped p, the second product keep ? p / (1 - p) : 0,
// the mask drawn at the TRUE key of each accumulator register (the second product walks a tile's keys in the planes' permuted order, the
// registers do not).  Without it the instruction stream holds no hash and ctx has the bits of the scoring call.
template <int NB, bool DROP>
__global__ __launch_bounds__(256, 2) void ass_kernel(AssArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ass_lds[];
  using G = AssGeom<NB>;
  constexpr int DP = G::DP, KS = G::KS, KP = G::KP, NST = NB;      // NST: 16-byte pieces per thread and half tile (8 DP / 256)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int sg = blockIdx.x / a.heads, h = blockIdx.x % a.heads, dh = a.dh;
  const AssSeq d = ass_find(a.seq, a.n_seq, sg, true);
  const int T = d.T;
  const int r0 = (sg - d.strip0) * AS_QS + wave * 32;
  const bool live = r0 < T;                                        // wave-uniform: a wave past the video only stages
  const int orow = min(r0 + li, T - 1);                            // clamped: such rows are never stored

  // Q fragments of both planes: k-step g, element j -> Q[query][16 g + 8 lh + j]
  bf16x8 qh[KS], ql[KS];
  {
    const char* qp = a.qp + (((int64_t)h * a.RP + d.prow0 + orow) * (2 * DP) + 8 * lh) * 2;
#pragma unroll
    for (int g = 0; g < KS; ++g) { qh[g] = ass_ld(qp + 32 * g); ql[g] = ass_ld(qp + 32 * g + 2 * DP); }
  }
  const char* Kt = a.kp + ((int64_t)h * a.RP + d.prow0) * (4 * DP);                   // tile c: + c * 256 DP bytes, contiguous
  const char* Vt = a.vp + ((int64_t)h * (a.RP / AS_KT) + d.prow0 / AS_KT) * (DP * 256);

  // staging of HALF a tile (128 DP bytes): thread -> NST pieces of 16 bytes, piece idx = 256 NB half + tid + 256 i of the tile
  u32x4 st[NST];
  auto gload = [&](const char* base, int c, int half) {
    const char* p = base + (int64_t)c * (DP * 256) + (256 * NB * half + tid) * 16;
#pragma unroll
    for (int i = 0; i < NST; ++i) st[i] = *reinterpret_cast<const u32x4*>(p + 4096 * i);
  };
  auto kwrite = [&](char* img, int half) {        // a K row is DP / 4 pieces
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = 256 * NB * half + tid + 256 * i;
      *reinterpret_cast<u32x4*>(img + (idx / (DP / 4)) * KP + (idx % (DP / 4)) * 16) = st[i];
    }
  };
  auto vwrite = [&](char* img, int half) {        // a V row is 16 pieces
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = 256 * NB * half + tid + 256 * i;
      *reinterpret_cast<u32x4*>(img + (idx >> 4) * ASS_VP + (idx & 15) * 16) = st[i];
    }
  };

  char* Kimg = ass_lds;
  char* Vimg = ass_lds + G::KIMG;
  const char* kfrag = Kimg + li * KP + 16 * lh;                    // + 32 sb KP + 32 g [+ 2 DP: lo]
  const char* vfrag = Vimg + li * ASS_VP + 16 * lh;                // + 32 b VP + 64 sb + 32 s [+ 128: lo]
  const int nt = (T + AS_KT - 1) / AS_KT;
  f32x16 o[NB], s0, s1;
  auto S = [&](int sb) -> f32x16& { return sb ? s1 : s0; };
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
  float m = -INFINITY, l = 0.f;                   // running maximum of the row; this lane half's share of the running sum
  constexpr float LOG2E = 1.4426950408889634f;
  const int64_t prow = d.row0 + orow;             // the packed row whose masks this lane draws (DROP)

  // first product over the k-steps [g0, g1)
  auto first = [&](int g0, int g1) {
#pragma unroll
    for (int g = g0; g < g1; ++g) {
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        const bf16x8 kh = ass_ld(kfrag + 32 * sb * KP + 32 * g), kl = ass_ld(kfrag + 32 * sb * KP + 32 * g + 2 * DP);
        S(sb) = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qh[g], S(sb), 0, 0, 0);
        S(sb) = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, ql[g], S(sb), 0, 0, 0);
        S(sb) = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kl, qh[g], S(sb), 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);          // keep the compiler from hoisting every step's reads (register budget)
    }
  };
  // second product of sub-tile sb: the weights split in registers, then 2 k-steps x NB blocks x 3 MFMAs
  auto accum = [&](int sb) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f32x8 p;
#pragma unroll
      for (int j = 0; j < 8; ++j) p[j] = S(sb)[8 * s + j];
      const bf16x8 ph = __builtin_convertvector(p, bf16x8);
      const bf16x8 pl = __builtin_convertvector(p - __builtin_convertvector(ph, f32x8), bf16x8);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const bf16x8 vh = ass_ld(vfrag + 32 * b * ASS_VP + 64 * sb + 32 * s), vl = ass_ld(vfrag + 32 * b * ASS_VP + 64 * sb + 32 * s + 128);
        o[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, ph, o[b], 0, 0, 0);
        o[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl, ph, o[b], 0, 0, 0);
        o[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, pl, o[b], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  gload(Kt, 0, 0); kwrite(Kimg, 0);
  gload(Kt, 0, 1); kwrite(Kimg, 1);
  for (int c = 0; c < nt; ++c) {
    const bool more = c + 1 < nt;
    __syncthreads();                              // K(c) is visible; every wave is done with V(c - 1)
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) S(sb)[r] = 0.f;
    gload(Vt, c, 0);                              // V(c) travels under the first product, half a tile at a time
    if (live) first(0, KS / 2);
    vwrite(Vimg, 0);
    gload(Vt, c, 1);
    if (live) first(KS / 2, KS);
    vwrite(Vimg, 1);
    __syncthreads();                              // V(c) is visible; every wave is done with K(c)
    if (more) gload(Kt, c + 1, 0);                // K(c + 1) travels under the softmax and the second product
    if (live) {
      if ((c + 1) * AS_KT > T) {                  // the video's last, partial tile: keys past T get the logit -inf
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
          for (int r = 0; r < 16; ++r) S(sb)[r] = (c * AS_KT + 32 * sb + as_crow(r, lh) < T) ? S(sb)[r] : -INFINITY;
      }
      float tm = -INFINITY;
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r) tm = fmaxf(tm, S(sb)[r]);
      tm = fmaxf(tm, __shfl_xor(tm, 32));
      const float mn = fmaxf(m, tm * a.scale);    // scale > 0: max_j (s_j scale) = (max_j s_j) scale, rounding is monotone
      const float f = __builtin_amdgcn_exp2f((m - mn) * LOG2E);
      float ps = 0.f;
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(S(sb)[r], a.scale, -mn) * LOG2E);
          ps += p;
          if (DROP) {
            S(sb)[r] = dropout_keep(a.seed, a.site, as_drop_idx(prow, a.heads, h, c * AS_KT + 32 * sb + as_crow(r, lh)), a.thr) ? p * a.keep_scale : 0.f;
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
          } else S(sb)[r] = p;
        }
      l = l * f + ps;
      m = mn;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] *= f;
      accum(0);
    }
    if (more) { kwrite(Kimg, 0); gload(Kt, c + 1, 1); }
    if (live) accum(1);
    if (more) kwrite(Kimg, 1);
  }

  if (!live) return;
  const float lt = l + __shfl_xor(l, 32);
  const int q = r0 + li;
  if (q >= T) return;
  float* cp = a.ctx + (d.row0 + q) * (int64_t)a.ldc + (int64_t)h * dh;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int dd = 32 * b + 8 * r4 + 4 * lh;    // as_crow(4 r4, lh): four consecutive columns; dh % 8 == 0 keeps a quad whole
      if (dd < dh) *reinterpret_cast<float4*>(cp + dd) = make_float4(o[b][4 * r4] / lt, o[b][4 * r4 + 1] / lt, o[b][4 * r4 + 2] / lt, o[b][4 * r4 + 3] / lt);
    }
  if (a.lse && lh == 0) a.lse[(d.row0 + q) * (int64_t)a.heads + h] = m + logf(lt);
  if (a.ml && lh == 0) a.ml[(d.row0 + q) * (int64_t)a.heads + h] = make_float2(m, lt);
}

struct AssLayout { size_t desc, qp, kp, vp, total; int64_t RP, strips; int nb; };

int ass_layout(const char* who, int D, int heads, int n_seq, const int32_t* off, int precision, AssLayout* L) {
  int64_t rp;
  SUMK_TRY(ass_check(who, D, heads, n_seq, off, precision, &rp, &L->strips, &L->nb));
  L->RP = rp;
  const size_t plane = (size_t)heads * (size_t)rp * (size_t)(32 * L->nb) * 4;   // hi + lo, 2 bytes each
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  L->desc = take((size_t)n_seq * sizeof(AssSeq));
  L->qp = take(plane); L->kp = take(plane); L->vp = take(plane);
  L->total = p;
  return SUMK_OK;
}

// tag: the profiler tag of the attention launch; ml / dl / site: the training form (ml null and dl.thr == 0: the scoring call)
template <int NB>
int ass_launch(const AssArgs& a, const AssLayout& L, int tag, hipStream_t stream) {
  prof_begin(SUMK_PROF_ATTN_STREAM_SPLIT_PLANES, stream);
  hipLaunchKernelGGL(ass_split_kernel<NB>, dim3((unsigned)(L.RP / AS_KT), (unsigned)a.heads), dim3(256), 0, stream, a);
  prof_end(SUMK_PROF_ATTN_STREAM_SPLIT_PLANES, stream);
  prof_begin(tag, stream);
  const int rc = a.thr ? as_launch<ass_kernel<NB, true>>(a, (unsigned)(L.strips * a.heads), AssGeom<NB>::LDS, stream)
                       : as_launch<ass_kernel<NB, false>>(a, (unsigned)(L.strips * a.heads), AssGeom<NB>::LDS, stream);
  prof_end(tag, stream);
  return rc;
}

int ass_run(const char* who, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int D, int heads, int n_seq,
            const int32_t* off_host, const int32_t* off_dev, float scale, int precision, float* ctx, int ldc, float* lse, float2* ml, Drop dl,
            uint32_t site, void* ws, int tag, hipStream_t stream) {
  SUMK_ARG(Q && K && V && ctx && off_dev && ws, "%s: null pointer", who);
  AssLayout L;
  SUMK_TRY(ass_layout(who, D, heads, n_seq, off_host, precision, &L));
  SUMK_ARG(heads <= 65535, "%s: n_heads=%d", who, heads);
  SUMK_ARG(ldq >= D && ldk >= D && ldv >= D && ldc >= D, "%s: leading dimensions (%d, %d, %d, %d) must be at least D=%d", who, ldq, ldk, ldv, ldc, D);
  SUMK_ARG(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldc % 4 == 0, "%s: leading dimensions (%d, %d, %d, %d) must be multiples of 4", who, ldq, ldk, ldv, ldc);
  SUMK_TRY(as_check_operands(who, (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)ctx | (uintptr_t)ws, "Q, K, V, ctx and the workspace", scale));
  AssArgs a;
  a.Q = Q; a.K = K; a.V = V; a.ctx = ctx; a.lse = lse; a.seq = (const AssSeq*)((char*)ws + L.desc);
  a.qp = (char*)ws + L.qp; a.kp = (char*)ws + L.kp; a.vp = (char*)ws + L.vp; a.RP = L.RP;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldc = ldc; a.dh = D / heads; a.heads = heads; a.n_seq = n_seq; a.scale = scale;
  a.ml = ml; a.seed = dl.seed; a.site = site; a.thr = dl.thr; a.keep_scale = dl.scale;
  hipLaunchKernelGGL(ass_setup_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, off_dev, n_seq, (AssSeq*)((char*)ws + L.desc));
  SUMK_TRY(L.nb == 1 ? ass_launch<1>(a, L, tag, stream) : L.nb == 2 ? ass_launch<2>(a, L, tag, stream) : ass_launch<4>(a, L, tag, stream));
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
}  // namespace

size_t attn_stream_split_ws_bytes(int D, int heads, int n_seq, const int32_t* off, int precision) {
  AssLayout L;
  return ass_layout("attn_stream_split", D, heads, n_seq, off, precision, &L) == SUMK_OK ? L.total : 0;
}

int launch_attn_stream_split(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int D, int heads, int n_seq,
                             const int32_t* off_host, const int32_t* off_dev, float scale, int precision, float* ctx, int ldc, float* lse,
                             void* ws, hipStream_t stream) {
  return ass_run("attn_stream_split", Q, ldq, K, ldk, V, ldv, D, heads, n_seq, off_host, off_dev, scale, precision, ctx, ldc, lse, nullptr,
                 make_drop(0.f, 0), 0u, ws, SUMK_PROF_ATTN_STREAM_SPLIT, stream);
}

int launch_attn_stream_split_train(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int D, int heads, int n_seq,
                                   const int32_t* off_host, const int32_t* off_dev, float scale, int precision, Drop dl, uint32_t site,
                                   float* ctx, int ldc, float* stats, void* ws, hipStream_t stream) {
  SUMK_ARG(stats && ((uintptr_t)stats & 7) == 0, "attn_stream_split_train: stats must be a non-null, 8-byte aligned (n_rows, n_heads, 2) array");
  SUMK_ARG(!dl.seed_dev, "attn_stream_split_train: no device seed word");
  return ass_run("attn_stream_split_train", Q, ldq, K, ldk, V, ldv, D, heads, n_seq, off_host, off_dev, scale, precision, ctx, ldc, nullptr,
                 (float2*)stats, dl, site, ws, SUMK_PROF_ATTN_STREAM_SPLIT_TRAIN, stream);
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_attn_stream_split_workspace_bytes(int32_t D, int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host,
                                                         int32_t precision) {
  return attn_stream_split_ws_bytes(D, n_heads, n_seq, seq_off_host, precision);
}

extern "C" int sumk_attn_stream_split(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                                      int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                                      int32_t precision, float* ctx, int32_t ldc, float* lse, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  SUMK_ARG(workspace, "attn_stream_split: null pointer");
  AssLayout L;
  SUMK_TRY(ass_layout("attn_stream_split", D, n_heads, n_seq, seq_off_host, precision, &L));
  if (workspace_bytes < L.total) { set_error("attn_stream_split: workspace %zu < required %zu", workspace_bytes, L.total); return SUMK_ERR_WORKSPACE; }
  return launch_attn_stream_split(Q, ldq, K, ldk, V, ldv, D, n_heads, n_seq, seq_off_host, seq_off_dev, scale, precision, ctx, ldc, lse,
                                  workspace, (hipStream_t)stream);
}

extern "C" int sumk_attn_stream_split_train(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                                            int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                            float scale, float dropout_p, uint64_t seed, uint32_t site, float* ctx, int32_t ldc, float* stats,
                                            void* workspace, size_t workspace_bytes, void* stream, int32_t precision) {
  const char* who = "attn_stream_split_train";
  SUMK_ARG(workspace, "%s: null pointer", who);
  SUMK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p=%g must lie in [0, 1)", who, (double)dropout_p);
  AssLayout L;
  SUMK_TRY(ass_layout(who, D, n_heads, n_seq, seq_off_host, precision, &L));
  if (workspace_bytes < L.total) { set_error("%s: workspace %zu < required %zu", who, workspace_bytes, L.total); return SUMK_ERR_WORKSPACE; }
  return launch_attn_stream_split_train(Q, ldq, K, ldk, V, ldv, D, n_heads, n_seq, seq_off_host, seq_off_dev, scale, precision,
                                        make_drop(dropout_p, seed), site, ctx, ldc, stats, workspace, (hipStream_t)stream);
}
