// Backward of the streaming multi-head attention (attn_stream.hip, training form) WITHOUT the (T x T) blocks, exact fp32, for gfx950.
//
//   s_ij = scale q_i . k_j     alpha_ij = softmax_j(s_ij)     a~_ij = keep_ij ? alpha_ij / (1 - p) : 0     ctx_i = sum_j a~_ij v_j
//   dV_j = sum_i a~_ij dctx_i  dA_ij = keep_ij ? (dctx_i . v_j) / (1 - p) : 0       delta_i = dctx_i . ctx_i (= sum_j dA_ij alpha_ij)
//   dS_ij = scale alpha_ij (dA_ij - delta_i)      dQ_i = sum_j dS_ij k_j      dK_j = sum_i dS_ij q_i
//
// per video and head of a packed batch; keep_ij = dropout_keep(seed, site, ((packed row i * heads + h) << 20) | j, thr), the index of
// tf_softmax_kernel (transformer.hip), so one seed gives the dense and the stream path the same masks.  The dense backward
// (tf_attn_core_bwd) reads alpha and dropout(alpha), heads x T x T floats each.  Here the weights are RECOMPUTED per tile from Q, K and
// the statistic the forward saved, the masks are regenerated in registers, and nothing of size T x T, or T x anything that grows with T,
// exists beyond inputs and outputs.  Workspace: the forward's descriptors + delta, 4 bytes per (row, head).
//
// The statistic is (m, l) per (row, head), 8 bytes: the row maximum and the sum of exp(s - m), not lse = m + log l.  alpha is recomputed as
// exp(fma(s, scale, -m)) * (1 / l), the forward's own expression.  With lse the exponent would carry the absolute rounding error of a
// number of several hundred (up to 3e-5 in the underflow and staircase cases of the tests) as a relative error of every weight of the row,
// as large as the whole budget of the gate; m is exact (it is one of the logits) and l is of order 1 .. T.
//
// Deterministic: no float atomics, no cooperative launch, no flag polled across workgroups.  Hence not the usual atomically accumulated
// dQ but TWO passes, each the forward's loop over again (seven products of 2 T^2 dh FLOP per head where the minimum is five):
//   asb_delta_kernel  delta[row, head] = dctx . ctx, one thread per (row, head), one chain over the head's columns
//   asb_dq_kernel     one workgroup (4 waves) per (query strip of 128 rows, head) walks the video's 64-key tiles in ascending order;
//                     a lane owns one query row.  S^T = K_tile (A) x Q^T (B) and dA^T = V_tile (A) x dctx^T (B) land in accumulator
//                     registers in the forward's layout, dS is formed there, and those registers are the B operand of
//                     dQ^T += K_tile^T dS^T (the forward's second product with the K image in place of the V image).
//   asb_dkv_kernel    one workgroup per (key strip of 128 rows, head) walks the video's 64-query tiles in ascending order, roles
//                     mirrored: a lane owns one key row, K and V fragments sit in registers, the Q and dctx tiles in LDS;
//                     S = Q_tile (A) x K^T (B), dA = dctx_tile (A) x V^T (B); the registers holding a~ and dS are the B operands of
//                     dV^T += dctx_tile^T a~ and dK^T += Q_tile^T dS.  m, 1 / l and delta of the tile's 64 queries come from LDS (they
//                     vary per accumulator register, not per lane).
// Both are ONE body (asb_pass): an "owner" strip whose two matrices X1, X2 live in registers as B fragments, and a "walked" tile whose
// two matrices Y1, Y2 live in LDS and serve as A operand of the first products and, transposed, of the accumulating ones.
//   pass   owner X1, X2    walked Y1, Y2    accumulators
//   dQ     Q, dctx         K, V             dQ^T += Y1^T dS^T
//   dK/dV  K, V            Q, dctx          dK^T += Y1^T dS,  dV^T += Y2^T a~
// Lane layout, the products (as_first, as_accum), the strip prologue and the owner-row store: attn_stream_common.h, shared with the
// forward.  This unit keeps its whole-tile double-image staging, the statistics in LDS and the formation of dS and a~.
//
// Walked rows past T are staged as zeros and their dS and a~ are set to 0 by a select in the video's last tile, so they contribute
// exactly 0; owner rows past T are the video's last row (clamped) and never stored.  NaN: a select, never a multiply, applies the masks,
// and a NaN of a video's Q, K, V or dctx reaches that video's gradients only (the walk never leaves the video).
//
// Sizes: strip 128 owner rows, tile 64 walked rows, NB = 1, 2, 4 blocks of 32 staged columns (dh <= 32 NB; dh = 256 does not fit the
// register file and is refused).  LDS per workgroup: two 64 x (32 NB + 4) images + 3 x 64 statistics = 67 KiB at dh = 128.  Staging: the
// next tile's two images travel in registers (4 NB float4 per thread) under the current tile's products; two barriers per tile.
// One wave per SIMD (__launch_bounds__(256, 1): 512 registers with the AGPRs).  By count at dh = 128: dQ pass 128 fragments + 64
// accumulators + 64 S / dA + 64 staging = 320; dK / dV pass 128 + 128 + 64 + 64 = 384.
// Compiler (hipcc -O3, gfx950) at dh = 128, VGPRs + AGPRs, spilled VGPRs (scratch bytes per lane), without / with dropout:
//   asb_dq_kernel<4>   256 + 163, none                 / 256 + 175, none
//   asb_dkv_kernel<4>  256 + 256, 48 (148 B)           / 256 + 256, 134 (492 B)
// The dK / dV pass fills the register file and spills: scripts/asm_loop_audit.py counts 18 .. 28 scratch instructions in its tile loop
// beside the loop's 512 MFMAs without dropout and 105 .. 156 with it (the hash's 64-bit temporaries); the dQ pass has none.  The smaller
// instances (NB = 1, 2) do not spill.  scripts/check_waterfalls.sh: 0.  Measured (scripts/attn_stream_train_timing.py, D = 1024, 8 heads,
// dropout 0.1): at T = 8192 the dQ pass takes 3.97 ms (6 T^2 D FLOP: 101 TFLOP/s) and the dK / dV pass 6.00 ms (8 T^2 D: 89 TFLOP/s).
// Tried at the compiler only, not run: both images double-buffered in the LDS that one workgroup per CU leaves free (134 KiB), staged
// half a tile at a time, one barrier per tile.  By count it frees 32 registers; the compiler then moves more fragment reads across the
// missing barrier and spills 117 (303 with dropout) in the dK / dV pass, so the single-buffered form above stayed.
#include "attn_stream_common.h"

namespace sumk {

namespace {

struct AsbArgs {
  const float* X1; const float* X2;       // the owner strip's matrices (registers): dQ pass Q, dctx; dK / dV pass K, V
  const float* Y1; const float* Y2;       // the walked tiles' matrices (LDS):       dQ pass K, V;    dK / dV pass Q, dctx
  float* O1; float* O2;                   // dQ pass: dQ, unused; dK / dV pass: dK, dV
  const float2* ml; const float* delta; const AsSeq* seq;
  int32_t ldx1, ldx2, ldy1, ldy2, ldo1, ldo2, dh, heads, n_seq; float scale;
  uint64_t seed; uint32_t site, thr; float keep_scale;
};

__global__ __launch_bounds__(256) void asb_delta_kernel(const float* __restrict__ ctx, int ldc, const float* __restrict__ dctx, int ldd,
                                                        float* __restrict__ delta, int64_t n, int heads, int dh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t row = i / heads; const int h = (int)(i % heads);
  const float* c = ctx + row * ldc + (int64_t)h * dh;
  const float* g = dctx + row * ldd + (int64_t)h * dh;
  float acc = 0.f;
  for (int d = 0; d < dh; d += 4) {
    const float4 a = *reinterpret_cast<const float4*>(c + d), b = *reinterpret_cast<const float4*>(g + d);
    acc = __builtin_fmaf(a.x, b.x, acc); acc = __builtin_fmaf(a.y, b.y, acc); acc = __builtin_fmaf(a.z, b.z, acc); acc = __builtin_fmaf(a.w, b.w, acc);
  }
  delta[i] = acc;
}

template <int NB, bool DKV, bool DROP>
__device__ __forceinline__ void asb_pass(const AsbArgs& a, float* lds) {
  using G = AsGeom<NB>;
  constexpr int P = G::P, C4 = G::C4, NST = 2 * NB;   // NST: float4 per thread and image (64 C4 / 256)
  const AsStrip w = as_strip(a.seq, a.n_seq, a.heads, a.dh);
  const AsSeq d = w.d;
  const int T = d.T, dh = a.dh, h = w.h, li = w.li, lh = w.lh, r0 = w.r0, orow = w.orow, tid = threadIdx.x;
  const bool live = w.live;
  const float* Y1h = a.Y1 + d.row0 * (int64_t)a.ldy1 + w.hcol;
  const float* Y2h = a.Y2 + d.row0 * (int64_t)a.ldy2 + w.hcol;

  // owner fragments: group g, MFMA j -> X[owner row][8 g + 4 lh + j]
  float xf1[4 * NB][4], xf2[4 * NB][4];
  {
    const float* p1 = a.X1 + (d.row0 + orow) * (int64_t)a.ldx1 + w.hcol;
    const float* p2 = a.X2 + (d.row0 + orow) * (int64_t)a.ldx2 + w.hcol;
#pragma unroll
    for (int g = 0; g < 4 * NB; ++g) {
      const int dc = 8 * g + 4 * lh;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f), u = t;
      if (live && dc < dh) { t = *reinterpret_cast<const float4*>(p1 + dc); u = *reinterpret_cast<const float4*>(p2 + dc); }
      xf1[g][0] = t.x; xf1[g][1] = t.y; xf1[g][2] = t.z; xf1[g][3] = t.w;
      xf2[g][0] = u.x; xf2[g][1] = u.y; xf2[g][2] = u.z; xf2[g][3] = u.w;
    }
  }
  // dQ pass: the statistic and delta of the lane's own query row
  float om = 0.f, oil = 0.f, odl = 0.f;
  if (!DKV) {
    const int64_t si = (d.row0 + orow) * (int64_t)a.heads + h;
    const float2 t = a.ml[si];
    om = t.x; oil = 1.0f / t.y; odl = a.delta[si];
  }

  float* img1 = lds;
  float* img2 = lds + G::IMG;
  float* sst = lds + 2 * G::IMG;                  // dK / dV pass: m, 1 / l, delta of the tile's 64 queries
  // staging of one 64-row tile of both walked matrices: thread -> NST float4 per image (row = idx / C4, float4 column = idx % C4,
  // idx = tid + 256 i); rows past T and columns past dh are zeros
  float4 st1[NST], st2[NST];
  float stm = 0.f, stil = 0.f, stdl = 0.f;
  auto gload = [&](int c) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = tid + 256 * i, r = idx / C4, c4 = idx % C4;
      const int wr = c * AS_KT + r;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f), u = t;
      if (4 * c4 < dh && wr < T) {
        t = *reinterpret_cast<const float4*>(Y1h + (int64_t)wr * a.ldy1 + 4 * c4);
        u = *reinterpret_cast<const float4*>(Y2h + (int64_t)wr * a.ldy2 + 4 * c4);
      }
      st1[i] = t; st2[i] = u;
    }
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
  auto swrite = [&]() {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = tid + 256 * i, r = idx / C4, c4 = idx % C4;
      *reinterpret_cast<float4*>(img1 + r * P + 4 * c4) = st1[i];
      *reinterpret_cast<float4*>(img2 + r * P + 4 * c4) = st2[i];
    }
    if (DKV && tid < AS_KT) { sst[tid] = stm; sst[AS_KT + tid] = stil; sst[2 * AS_KT + tid] = stdl; }
  };

  const int nt = (T + AS_KT - 1) / AS_KT;
  f32x16 o1[NB], o2[DKV ? NB : 1], s[2], da[2];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) o1[b][r] = 0.f;
#pragma unroll
  for (int b = 0; b < (DKV ? NB : 1); ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) o2[b][r] = 0.f;

  gload(0);
  for (int c = 0; c < nt; ++c) {
    __syncthreads();                              // every wave is done with tile c - 1
    swrite();
    __syncthreads();                              // tile c is visible
    if (c + 1 < nt) gload(c + 1);                 // tile c + 1 travels under the products of tile c
    if (!live) continue;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[sb][r] = 0.f; da[sb][r] = 0.f; }
    as_first<NB, 0, 4 * NB>(img1, li, lh, xf1, s[0], s[1]);
    as_first<NB, 0, 4 * NB>(img2, li, lh, xf2, da[0], da[1]);
    const bool partial = (c + 1) * AS_KT > T;     // the video's last tile: walked rows past T contribute exactly 0
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tr = 32 * sb + as_crow(r, lh), wr = c * AS_KT + tr;       // walked row: inside the tile, inside the video
        float m = om, il = oil, dl = odl;
        if (DKV) { m = sst[tr]; il = sst[AS_KT + tr]; dl = sst[2 * AS_KT + tr]; }
        const float alpha = expf(__builtin_fmaf(s[sb][r], a.scale, -m)) * il;
        float dA = da[sb][r], at = alpha;
        if (DROP) {
          const uint64_t idx = DKV ? as_drop_idx(d.row0 + wr, a.heads, h, r0 + li) : as_drop_idx(d.row0 + orow, a.heads, h, wr);
          const bool keep = dropout_keep(a.seed, a.site, idx, a.thr);
          dA = keep ? dA * a.keep_scale : 0.f;
          at = keep ? alpha * a.keep_scale : 0.f;
        }
        float ds = alpha * (dA - dl) * a.scale;
        if (partial && wr >= T) { ds = 0.f; at = 0.f; }
        da[sb][r] = ds; s[sb][r] = at;
        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    as_accum<NB>(img1, 0, li, lh, da[0], o1);
    as_accum<NB>(img1, 1, li, lh, da[1], o1);
    if (DKV) {
      as_accum<NB>(img2, 0, li, lh, s[0], o2);
      as_accum<NB>(img2, 1, li, lh, s[1], o2);
    }
  }

  if (!live || r0 + li >= T) return;
  as_store_row<NB>(w, dh, a.O1, a.ldo1, o1);
  if constexpr (DKV) as_store_row<NB>(w, dh, a.O2, a.ldo2, o2);
}

template <int NB, bool DROP>
__global__ __launch_bounds__(256, 1) void asb_dq_kernel(AsbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float asb_lds[];
  asb_pass<NB, false, DROP>(a, asb_lds);
}
template <int NB, bool DROP>
__global__ __launch_bounds__(256, 1) void asb_dkv_kernel(AsbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float asb_lds[];
  asb_pass<NB, true, DROP>(a, asb_lds);
}

template <int NB> constexpr int ASB_LDS = (2 * AsGeom<NB>::IMG + 3 * AS_KT) * 4;

constexpr int ASB_MAX_DH = 128;
}  // namespace

int attn_stream_bwd_check(int D, int heads, int n_seq, const int32_t* off, int64_t* strips) {
  SUMK_TRY(attn_stream_check(D, heads, n_seq, off, strips));
  const int dh = D / heads;
  SUMK_ARG(dh <= ASB_MAX_DH, "attn_stream_backward: head width %d (D=%d, n_heads=%d) must be at most %d", dh, D, heads, ASB_MAX_DH);
  return SUMK_OK;
}

void launch_attn_stream_bwd_delta(const float* ctx, int ldc, const float* dctx, int ldd, float* delta, int64_t n_rows, int heads, int dh,
                                  hipStream_t stream) {
  const int64_t nrh = n_rows * heads;
  prof_begin(SUMK_PROF_ATTN_STREAM_BWD_DELTA, stream);
  hipLaunchKernelGGL(asb_delta_kernel, dim3((unsigned)((nrh + 255) / 256)), dim3(256), 0, stream, ctx, ldc, dctx, ldd, delta, nrh, heads, dh);
  prof_end(SUMK_PROF_ATTN_STREAM_BWD_DELTA, stream);
}

size_t attn_stream_bwd_ws_bytes(int heads, int n_seq, int64_t n_rows) {
  return attn_stream_ws_bytes(n_seq) + align_up((size_t)n_rows * (size_t)heads * sizeof(float), 256);
}

int launch_attn_stream_bwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* ctx, int ldc,
                           const float* dctx, int ldd, const float* stats, int D, int heads, int n_seq, const int32_t* off_host,
                           const int32_t* off_dev, float scale, Drop dl, uint32_t site, float* dQ, int lddq, float* dK, int lddk, float* dV,
                           int lddv, void* ws, hipStream_t stream) {
  SUMK_ARG(Q && K && V && ctx && dctx && stats && dQ && dK && dV && off_dev && ws, "attn_stream_backward: null pointer");
  int64_t strips;
  SUMK_TRY(attn_stream_bwd_check(D, heads, n_seq, off_host, &strips));
  const int lds[8] = {ldq, ldk, ldv, ldc, ldd, lddq, lddk, lddv};
  for (int i = 0; i < 8; ++i) {
    SUMK_ARG(lds[i] >= D, "attn_stream_backward: leading dimension %d (argument %d of 8) must be at least D=%d", lds[i], i, D);
    SUMK_ARG(lds[i] % 4 == 0, "attn_stream_backward: leading dimension %d (argument %d of 8) must be a multiple of 4", lds[i], i);
  }
  SUMK_ARG(((uintptr_t)stats & 7) == 0, "attn_stream_backward: stats must be 8-byte aligned");
  SUMK_TRY(as_check_operands("attn_stream_backward", (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)ctx | (uintptr_t)dctx | (uintptr_t)dQ | (uintptr_t)dK | (uintptr_t)dV,
                             "Q, K, V, ctx, dctx, dQ, dK and dV", scale));
  SUMK_ARG(!dl.seed_dev, "attn_stream_backward: no device seed word");
  const int64_t n_rows = off_host[n_seq];
  float* delta = (float*)((char*)ws + attn_stream_ws_bytes(n_seq));
  attn_stream_setup(off_dev, n_seq, ws, stream);
  launch_attn_stream_bwd_delta(ctx, ldc, dctx, ldd, delta, n_rows, heads, D / heads, stream);
  AsbArgs a;
  a.ml = (const float2*)stats; a.delta = delta; a.seq = (const AsSeq*)ws;
  a.dh = D / heads; a.heads = heads; a.n_seq = n_seq; a.scale = scale;
  a.seed = dl.seed; a.site = site; a.thr = dl.thr; a.keep_scale = dl.scale;
  const unsigned blocks = (unsigned)(strips * heads);
  a.X1 = Q; a.ldx1 = ldq; a.X2 = dctx; a.ldx2 = ldd; a.Y1 = K; a.ldy1 = ldk; a.Y2 = V; a.ldy2 = ldv;
  a.O1 = dQ; a.ldo1 = lddq; a.O2 = nullptr; a.ldo2 = 0;
  prof_begin(SUMK_PROF_ATTN_STREAM_BWD_DQ, stream);
  SUMK_TRY(as_dispatch<4>(a.dh, a.thr != 0, [&](auto nb, auto drop) {
    return as_launch<asb_dq_kernel<nb(), drop()>>(a, blocks, ASB_LDS<nb()>, stream);
  }));
  prof_end(SUMK_PROF_ATTN_STREAM_BWD_DQ, stream);
  a.X1 = K; a.ldx1 = ldk; a.X2 = V; a.ldx2 = ldv; a.Y1 = Q; a.ldy1 = ldq; a.Y2 = dctx; a.ldy2 = ldd;
  a.O1 = dK; a.ldo1 = lddk; a.O2 = dV; a.ldo2 = lddv;
  prof_begin(SUMK_PROF_ATTN_STREAM_BWD_DKV, stream);
  SUMK_TRY(as_dispatch<4>(a.dh, a.thr != 0, [&](auto nb, auto drop) {
    return as_launch<asb_dkv_kernel<nb(), drop()>>(a, blocks, ASB_LDS<nb()>, stream);
  }));
  prof_end(SUMK_PROF_ATTN_STREAM_BWD_DKV, stream);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_attn_stream_backward_workspace_bytes(int32_t D, int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host) {
  if (attn_stream_bwd_check(D, n_heads, n_seq, seq_off_host) != SUMK_OK) return 0;
  return attn_stream_bwd_ws_bytes(n_heads, n_seq, seq_off_host[n_seq]);
}

extern "C" int sumk_attn_stream_backward(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, const float* ctx,
                                         int32_t ldc, const float* dctx, int32_t ldd, const float* stats, int32_t D, int32_t n_heads,
                                         int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale, float dropout_p,
                                         uint64_t seed, uint32_t site, float* dQ, int32_t lddq, float* dK, int32_t lddk, float* dV,
                                         int32_t lddv, void* workspace, size_t workspace_bytes, void* stream) {
  SUMK_ARG(workspace, "attn_stream_backward: null pointer");
  SUMK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "attn_stream_backward: dropout_p=%g must lie in [0, 1)", (double)dropout_p);
  SUMK_TRY(attn_stream_bwd_check(D, n_heads, n_seq, seq_off_host));
  const size_t need = attn_stream_bwd_ws_bytes(n_heads, n_seq, seq_off_host[n_seq]);
  if (workspace_bytes < need) { set_error("attn_stream_backward: workspace %zu < required %zu", workspace_bytes, need); return SUMK_ERR_WORKSPACE; }
  return launch_attn_stream_bwd(Q, ldq, K, ldk, V, ldv, ctx, ldc, dctx, ldd, stats, D, n_heads, n_seq, seq_off_host, seq_off_dev, scale,
                                make_drop(dropout_p, seed), site, dQ, lddq, dK, lddk, dV, lddv, workspace, (hipStream_t)stream);
}
