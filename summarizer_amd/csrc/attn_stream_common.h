// What the streaming attention units share (attn_stream.hip: forward; attn_stream_bwd.hip: backward): the tile geometry, the per-video
// descriptor, the two MFMA products with their lane layout, the strip prologue and the owner-row store around them, and the host path
// that checks and launches.
//
// Both units' kernels are one workgroup (4 waves) per (strip of AS_QS = 128 OWNER rows, head); block = strip * heads + head, so the
// heads of a strip run side by side.  A wave owns 32 whole owner rows, a lane one of them; the workgroup WALKS the video's tiles of
// AS_KT = 64 rows in ascending order.  The owner rows' matrices sit in registers as B fragments, a walked tile's matrices in LDS as
// images of 64 x P floats (P = 32 NB + 4: the pitch that makes the ds_read_b128 of both products below conflict-free).
//   unit / pass       owner rows     walked rows
//   forward, dQ       queries        keys
//   dK / dV           keys           queries
//
// Lane layout (v_mfma_f32_32x32x2_f32 for every product; lane = (li = lane & 31, lh = lane >> 5)):
//   First product (as_first)  acc^T = img (A) x X_owner^T (B): A[row li][k lh] = img[walked row 32 sb + li][d], B[k lh][col li] =
//     X[owner row li][d]; one ds_read_b128 of an image row feeds four MFMAs, so MFMA j of group g contracts d = 8 g + j (lh 0) then
//     8 g + 4 + j (lh 1), groups ascending.  Accumulator register r of sub-tile sb then holds, for OWNER row li, walked row
//     32 sb + as_crow(r, lh), as_crow(r, lh) = (r & 3) + 8 (r >> 2) + 4 lh: a lane owns one owner row and 32 of the tile's 64 walked
//     rows, its partner lane ^ 32 the others.
//   Accumulating product (as_accum)  out^T[d][owner] += img^T[d][walked] w^T[walked][owner]: with f32 operands that accumulator register
//     IS the B operand of MFMA step (sb, r) -- B[k lh][col li] = w[owner li][walked 32 sb + as_crow(r, lh)] -- so the weights are never
//     converted, never go through LDS and never change lane.  The matching A value is img[32 sb + as_crow(r, lh)][d] with d chosen by
//     the lane: d = (b % W) + W li + 32 W (b / W) for accumulator block b, W = min(NB, 4), so that ONE ds_read_b128 (W = 4) of an image
//     row feeds the MFMAs of four blocks.  Block b register r of lane (li, lh) is out[owner li][d = as_ocol(b, r, lh)]: anything
//     per owner row (the forward's running rescale) is a per-lane multiply.
// Both products read their fragments one step ahead of the MFMAs that consume them, with a scheduling barrier per step: left alone,
// the compiler hoists every ds_read of a phase and spills (as_stream_kernel<4, false> sits at 239 of 256 VGPRs).
//
// How the shared bodies are written is part of that register budget (checked against the compiler's output, instance by instance:
// scripts/asm_loop_audit.py and the .vgpr_count / .vgpr_spill_count metadata):
//   * as_first / as_accum take the image pointer and li / lh BY REFERENCE, as the lambdas they replace captured them; by value the
//     compiler reassociates the fragment addresses and every instance of the forward grows by 3 .. 10 VGPRs (DROP instances spill more).
//   * a sub-tile of logits / weights is passed as ONE f32x16 per argument, and the forward keeps its two as two objects.  An f32x16[2]
//     handed to these templates is promoted to a single 32-wide vector: a 32-register tuple, +17 VGPRs and spills in
//     as_stream_kernel<4, false>.
//   * the owner-fragment LOAD stays in each kernel (a dozen lines, twice): moved into a template here, with any signature, it reorders
//     the loads' phis and as_stream_kernel<4, true> spills 185 VGPRs instead of 85.
//
// Head width: NB = 1, 2, 4, 8 blocks of 32 staged columns (dh <= 32 NB; the columns dh .. 32 NB - 1 of every matrix are staged as
// zeros, so dh = 36 or 100 take the same loops as 128: their padded k-steps add fma(0, 0, acc)).  Owner rows past T are the video's
// last row (clamped) and never stored.
#pragma once
#include "gemm_device.h"
#include <math.h>
#include <type_traits>

namespace sumk {

constexpr int AS_KT = 64;                 // rows of a walked tile (keys in the forward and the dQ pass, queries in the dK / dV pass)
constexpr int AS_QS = 128;                // rows per strip a workgroup owns: 4 waves x 32
constexpr int AS_MAX_T = 1 << 20;
constexpr int AS_MAX_SEQ = 65535;

struct AsSeq { int64_t row0; int32_t T; int32_t strip0; };   // first packed row, frames, first strip of the video

template <int NB> struct AsGeom {
  static constexpr int DP = 32 * NB, P = DP + 4;            // staged columns; LDS pitch
  static constexpr int C4 = DP / 4;                         // float4 columns of a tile row
  static constexpr int W = NB < 4 ? NB : 4, NQ = NB / W;    // accumulator blocks one fragment read feeds; reads per step
  static constexpr int IMG = AS_KT * P;                     // floats of one image
};

// row of accumulator register r inside a 32 x 32 block for lane half lh
__device__ __forceinline__ int as_crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }
// column of the owner row's output that register r of accumulator block b holds
template <int NB> __device__ __forceinline__ int as_ocol(int b, int r, int lh) {
  constexpr int W = AsGeom<NB>::W;
  return (b % W) + W * as_crow(r, lh) + 32 * W * (b / W);
}

template <int W> struct AsVec;
template <> struct AsVec<1> { float v[1]; __device__ __forceinline__ void load(const float* p) { v[0] = *p; } };
template <> struct AsVec<2> { float v[2]; __device__ __forceinline__ void load(const float* p) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; } };
template <> struct AsVec<4> { float v[4]; __device__ __forceinline__ void load(const float* p) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; } };

// index of the dropout mask of weight (packed query row, head, key): the one tf_softmax_kernel (transformer.hip) uses
__device__ __forceinline__ uint64_t as_drop_idx(int64_t packed_row, int heads, int h, int key) {
  return ((uint64_t)(packed_row * heads + h) << 20) | (uint64_t)key;
}

// ------------------------------------------------------------------------------------------- the strip walk
// where a lane stands: its workgroup's video and head, its wave's 32 owner rows, its own owner row
struct AsStrip {
  AsSeq d; int h, li, lh;
  int r0; bool live;          // the wave's first owner row inside the video; wave-uniform: a wave past the video only stages
  int orow; int64_t hcol;     // the lane's owner row (clamped: such rows are never stored); first column of the head
};
__device__ __forceinline__ AsStrip as_strip(const AsSeq* seq, int n_seq, int heads, int dh) {
  AsStrip s;
  const int blk = blockIdx.x;
  const int sg = blk / heads;
  s.h = blk % heads;
  int lo = 0, hi = n_seq - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seq[mid].strip0 <= sg) lo = mid; else hi = mid - 1; }
  s.d = seq[lo];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  s.li = lane & 31; s.lh = lane >> 5;
  s.r0 = (sg - s.d.strip0) * AS_QS + wave * 32;
  s.live = s.r0 < s.d.T;
  s.orow = min(s.r0 + s.li, s.d.T - 1);
  s.hcol = (int64_t)s.h * dh;
  return s;
}

// First product: acc^T += img (A) x frag^T (B) over the groups [G0, G0 + N) of the 4 NB; the image fragments of group g + 1 are read
// under the MFMAs of group g.  Every group runs: the columns past dh are zeros in both operands.
template <int NB, int G0, int N>
__device__ __forceinline__ void as_first(float* const& img, const int& li, const int& lh, const float (&xf)[4 * NB][4], f32x16& acc0, f32x16& acc1) {
  constexpr int P = AsGeom<NB>::P;
  float4 kf[2], kn[2];
  auto kread = [&](int g, float4 (&dst)[2]) {
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) dst[sb] = *reinterpret_cast<const float4*>(img + (32 * sb + li) * P + 8 * g + 4 * lh);
  };
  auto quad = [&](const float4& k, const float (&x)[4], f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k.x, x[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k.y, x[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k.z, x[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k.w, x[3], acc, 0, 0, 0);
  };
  kread(G0, kf);
#pragma unroll
  for (int gi = 0; gi < N; ++gi) {
    const int g = G0 + gi;
    if (gi + 1 < N) kread(g + 1, kn);
    quad(kf[0], xf[g], acc0);
    quad(kf[1], xf[g], acc1);
    kf[0] = kn[0]; kf[1] = kn[1];
    __builtin_amdgcn_sched_barrier(0);          // keep the compiler from hoisting every group's reads (register budget)
  }
}

// Accumulating product: out^T += img^T w^T over the 16 steps of sub-tile sb; the image fragments of step r + 1 are read under the MFMAs
// of step r
template <int NB, int NO>
__device__ __forceinline__ void as_accum(float* const& img, int sb, const int& li, const int& lh, const f32x16& w, f32x16 (&out)[NO]) {
  constexpr int P = AsGeom<NB>::P, W = AsGeom<NB>::W, NQ = AsGeom<NB>::NQ;
  AsVec<W> vc[NQ], vn[NQ];
  auto vread = [&](int r, AsVec<W> (&dst)[NQ]) {
    const float* vp = img + (32 * sb + as_crow(r, lh)) * P + W * li;
#pragma unroll
    for (int bq = 0; bq < NQ; ++bq) dst[bq].load(vp + 32 * W * bq);
  };
  vread(0, vc);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (r + 1 < 16) vread(r + 1, vn);
#pragma unroll
    for (int bq = 0; bq < NQ; ++bq)
#pragma unroll
      for (int bb = 0; bb < W; ++bb)
        out[bq * W + bb] = __builtin_amdgcn_mfma_f32_32x32x2f32(vc[bq].v[bb], w[r], out[bq * W + bb], 0, 0, 0);
#pragma unroll
    for (int bq = 0; bq < NQ; ++bq) vc[bq] = vn[bq];
    __builtin_amdgcn_sched_barrier(0);
  }
}

// the lane's owner row of O (leading dimension ld) = its NB accumulator blocks [/ div]; the caller has checked that the row is inside the video
template <int NB, bool DIV = false>
__device__ __forceinline__ void as_store_row(const AsStrip& s, int dh, float* O, int ld, const f32x16 (&o)[NB], float div = 1.f) {
  const int q = s.r0 + s.li;
  float* p = O + (s.d.row0 + q) * (int64_t)ld + s.hcol;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dd = as_ocol<NB>(b, r, s.lh);
      if (dd < dh) p[dd] = DIV ? o[b][r] / div : o[b][r];
    }
}

// ------------------------------------------------------------------------------------------- host
// the per-video descriptors (attn_stream_ws_bytes(n_seq) bytes at `ws`) both units' kernels read; strips of AS_QS rows
void attn_stream_setup(const int32_t* off_dev, int n_seq, void* ws, hipStream_t stream);

// what both units ask of their matrices and of the scale: `misaligned` = the OR of the matrices' addresses, `names` = how the message
// lists them
inline int as_check_operands(const char* who, uintptr_t misaligned, const char* names, float scale) {
  SUMK_ARG((misaligned & 15) == 0, "%s: %s must be 16-byte aligned", who, names);
  SUMK_ARG(scale > 0.f && scale < INFINITY, "%s: scale=%g must be positive and finite", who, (double)scale);
  return SUMK_OK;
}

// f(NB, DROP) as integral constants for the instance that serves head width dh <= 32 MAX_NB with or without dropout of the weights
template <int MAX_NB, class F>
int as_dispatch(int dh, bool drop, F&& f) {
  auto width = [&](auto dr) {
    if (dh <= 32) return f(std::integral_constant<int, 1>{}, dr);
    if (dh <= 64) return f(std::integral_constant<int, 2>{}, dr);
    if constexpr (MAX_NB >= 8) { if (dh > 128) return f(std::integral_constant<int, 8>{}, dr); }
    return f(std::integral_constant<int, 4>{}, dr);
  };
  return drop ? width(std::true_type{}) : width(std::false_type{});
}

// one workgroup of 256 threads per (strip, head) with `lds` bytes of dynamic LDS, opted into past the default limit
template <auto Kernel, class Args>
int as_launch(const Args& a, unsigned blocks, int lds, hipStream_t stream) {
  if (lds > 64 * 1024) SUMK_TRY(lds_opt_in<Kernel>(lds));
  hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(256), lds, stream, a);
  return SUMK_OK;
}

}  // namespace sumk
