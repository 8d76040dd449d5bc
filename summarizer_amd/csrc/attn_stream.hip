// Multi-head attention WITHOUT the (T x T) logits: the streaming, exact-fp32 form of tf_attn_core_fwd (transformer.hip) for long videos.
//
//   ctx[rows of v, h dh : (h + 1) dh] = softmax_j(scale Q_h K_h^T) V_h          per video v and head h of a packed batch, no mask
//
// tf_attn_core_fwd stores heads x T x T logits per video (2.1 GB at T = 8192, 8 heads) and makes four passes over them.  Here a logit
// lives in an MFMA accumulator register from the first product to the second: nothing of size T x T, or T x anything that grows with T,
// exists beyond the inputs and the outputs.  Workspace: one 16-byte descriptor per video.
//
// Launches of one call (both on the caller's stream, nothing else: the call captures into a HIP graph):
//   as_setup_kernel    per-video descriptors (first row, frames, first query strip) from the device offsets
//   as_stream_kernel   one workgroup (4 waves) per (query strip of 128 rows, head); block = strip * heads + head, so the heads of a strip
//                      run side by side and a head's K / V tiles are shared through L2 by the strips running at that time.  A wave owns
//                      32 WHOLE query rows; the workgroup walks the video's 64-key tiles in ascending order.  No column split.
// No cooperative launch, no flag polled across workgroups, no atomics: bit-deterministic.
//
// Lane layout, the two products (S^T = K_tile x Q_strip^T, the swapped product of rs_stream_kernel, then O^T += V^T P^T with the
// accumulator registers of the first as B operand of the second) and the strip prologue: attn_stream_common.h, shared with the backward.
// Owner rows are queries, walked rows keys.  What is the forward's own:
//   Row maximum: 31 fmax in the lane + one exchange with lane ^ 32.  Row sum: each lane half keeps its own partial (same rescale factor
//     in both), joined once after the walk.  The running rescale of O is a per-lane multiply (a lane owns one query row).
//
// Online softmax per tile, UNCONDITIONALLY (no deferred-max threshold, hence no rare data-dependent branch): m' = max(m, scale max_j s_j),
// f = exp(m - m'), p_j = exp(fma(s_j, scale, -m')) (the dense kernel's expression), l = l f + sum p, O = O f + P V; at the end O / l and
// lse = m + log(l).  m starts at -inf: the first tile's f is exp(-inf) = 0.  Keys past T get the logit -inf (p = 0 exactly) and their V
// rows are staged as zeros; their K rows and the query rows past T are the video's last row (clamped) and such queries are never stored.
//
// Head width: one kernel body, instantiated for NB = 1, 2, 4, 8 blocks of 32 columns (dh <= 32 NB; the columns dh .. 32 NB - 1 of Q, K
// and V are staged as zeros, so dh = 36 or 100 take the same loop as 128: their padded k-steps add fma(0, 0, acc)).  Per workgroup:
//   dh      NB   LDS: K tile + V tile, 64 x (32 NB + 4) floats each    registers per lane: Q 16 NB + O 16 NB + S 32 + staging 4 NB + fragments
//   128     4    66 KiB  -> 2 workgroups per CU (132 of 160 KiB)         64 + 64 + 32 + 16 + 16 = 192 by count; the compiler takes 239 of 256, no
//                                                                       spill: 2 waves per SIMD
//   256     8    130 KiB -> 1 workgroup per CU                          128 + 128 + 32 + 32 + 24 = 344 of 512 by count (1 wave per SIMD); the compiler
//                                                                       fills 256 VGPRs + 256 AGPRs and still spills 113 to scratch: correct (the
//                                                                       strips test runs it), not yet tuned: 103 TFLOP/s at T = 8192
// K and V are single-buffered in LDS: two 64 x 256 tiles are 64 KiB each, so dh = 256 could not double-buffer both at 64 keys.  The
// next tile travels in the staging registers instead, HALF a tile at a time (a whole one would not fit the budget at dh = 128): V(c)
// is loaded under the first product of tile c, K(c + 1) under the softmax and the second product.  Two barriers per tile; at dh <= 128
// the second workgroup of the CU fills them.
//
// Vector-ALU work per tile and lane beside the 64 NB MFMAs (fp32 MFMA issues on the vector ALU here, so it adds to them): 32 fmax,
// 1 multiply + 1 fmax + 1 exchange, 32 fma + 32 exp + 32 adds, 16 NB multiplies of O.  exp is the accurate expf (about 15
// instructions), which makes this roughly 700 instructions x 4 cycles against 256 MFMAs x 64 cycles at dh = 128: about 17 % by count, not
// the 5 % a bare v_exp_f32 would give.  Measured (scripts/attn_stream_timing.py, D = 1024, 8 heads): 122 TFLOP/s at T = 8192, 129 at
// T = 65 536 -- the two waves of a SIMD overlap one's softmax with the other's MFMAs.
//
// The training form (sumk_attn_stream_train; its backward: attn_stream_bwd.hip) is the same kernel with two additions.  The statistic of
// a row, (m, l) per (row, head), is written whenever a.ml is given.  DROP instances drop the weights: the running sum l takes the
// undropped p, the B operand of the second product keep ? p / (1 - p) : 0 with keep = dropout_keep(seed, site, ((packed row * heads + h)
// << 20) | key, thr), the index of tf_softmax_kernel.  Without dropout the non-DROP instances run: no hash in the instruction stream, ctx
// has the bits of the inference call.  The hash (three 64-bit multiplies per weight) costs registers: as_stream_kernel<4, true> takes all
// 256 VGPRs of its two-waves-per-SIMD budget and spills 85 (27 scratch instructions in the tile loop beside its 256 MFMAs); measured
// 95 TFLOP/s at T = 8192 against 122 without dropout.
#include "attn_stream_common.h"
#include <algorithm>

namespace sumk {

namespace {
constexpr int AS_MAX_DH = 256;

struct AsArgs {
  const float* Q; const float* K; const float* V; float* ctx; float* lse; const AsSeq* seq;
  int32_t ldq, ldk, ldv, ldc, dh, heads, n_seq; float scale;
  // the training form: the statistic (m, l) per (row, head) for the backward, and the dropout of the weights (DROP instances only)
  float2* ml; uint64_t seed; uint32_t site, thr; float keep_scale;
};

__global__ void as_setup_kernel(const int32_t* off, int n_seq, AsSeq* seq) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  int strip0 = 0;
  for (int q = 0; q < s; ++q) strip0 += (off[q + 1] - off[q] + AS_QS - 1) / AS_QS;
  AsSeq d; d.row0 = off[s]; d.T = off[s + 1] - off[s]; d.strip0 = strip0;
  seq[s] = d;
}

// DROP: the training form with dropout of the weights -- the running sum takes the undropped p, the second product keep ? p / (1 - p) : 0
// (mask index as tf_softmax_kernel's).  Without it the instruction stream holds no hash and ctx has the bits of the inference call.
template <int NB, bool DROP>
__global__ __launch_bounds__(256, NB <= 4 ? 2 : 1) void as_stream_kernel(AsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float as_lds[];
  using G = AsGeom<NB>;
  constexpr int P = G::P, C4 = G::C4, NST = NB;  // NST: float4 per thread and half tile (32 C4 / 256)
  const AsStrip w = as_strip(a.seq, a.n_seq, a.heads, a.dh);
  const AsSeq d = w.d;
  const int T = d.T, dh = a.dh, h = w.h, li = w.li, lh = w.lh, tid = threadIdx.x;
  const bool live = w.live;
  const float* Kh = a.K + d.row0 * (int64_t)a.ldk + w.hcol;
  const float* Vh = a.V + d.row0 * (int64_t)a.ldv + w.hcol;

  // Q fragments: group g, MFMA j -> Q[query][8 g + 4 lh + j]
  float qf[4 * NB][4];
  {
    const float* qp = a.Q + d.row0 * (int64_t)a.ldq + w.hcol + (int64_t)w.orow * a.ldq;
#pragma unroll
    for (int g = 0; g < 4 * NB; ++g) {
      const int dc = 8 * g + 4 * lh;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live && dc < dh) t = *reinterpret_cast<const float4*>(qp + dc);
      qf[g][0] = t.x; qf[g][1] = t.y; qf[g][2] = t.z; qf[g][3] = t.w;
    }
  }

  // staging of HALF a 64-row tile (the whole one would not fit the register budget): thread -> NST float4 of rows 32 half .. 32 half + 31
  // (row = 32 half + idx / C4, float4 column = idx % C4, idx = tid + 256 i)
  float4 st[NST];
  auto gload = [&](const float* base, int ld, int c, int half, bool zero_rows) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = tid + 256 * i, r = 32 * half + idx / C4, c4 = idx % C4;
      const int key = c * AS_KT + r;
      const bool ok = 4 * c4 < dh && !(zero_rows && key >= T);
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok) t = *reinterpret_cast<const float4*>(base + (int64_t)min(key, T - 1) * ld + 4 * c4);
      st[i] = t;
    }
  };
  auto swrite = [&](float* img, int half) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = tid + 256 * i, r = 32 * half + idx / C4, c4 = idx % C4;
      *reinterpret_cast<float4*>(img + r * P + 4 * c4) = st[i];
    }
  };

  float* Kimg = as_lds;
  float* Vimg = as_lds + G::IMG;
  const int nt = (T + AS_KT - 1) / AS_KT;
  // s0, s1: the tile's two sub-tiles of logits, then weights.  Two objects, not s[2]: beside the shared products the compiler keeps
  // such an array as ONE 32-wide vector (a 32-register tuple) and as_stream_kernel<4, false> spills (attn_stream_common.h)
  f32x16 o[NB], s0, s1;
  auto S = [&](int sb) -> f32x16& { return sb ? s1 : s0; };
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
  float m = -INFINITY, l = 0.f;                   // running maximum of the row; this lane half's share of the running sum
  const int64_t prow = d.row0 + w.orow;           // the packed row whose masks this lane draws (DROP)

  gload(Kh, a.ldk, 0, 0, false); swrite(Kimg, 0);
  gload(Kh, a.ldk, 0, 1, false); swrite(Kimg, 1);
  for (int c = 0; c < nt; ++c) {
    const bool more = c + 1 < nt;
    __syncthreads();                              // K(c) is visible; every wave is done with V(c - 1)
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) S(sb)[r] = 0.f;
    gload(Vh, a.ldv, c, 0, true);                 // V(c) travels under the first product, half a tile at a time
    if (live) as_first<NB, 0, 2 * NB>(Kimg, li, lh, qf, s0, s1);
    swrite(Vimg, 0);
    gload(Vh, a.ldv, c, 1, true);
    if (live) as_first<NB, 2 * NB, 2 * NB>(Kimg, li, lh, qf, s0, s1);
    swrite(Vimg, 1);
    __syncthreads();                              // V(c) is visible; every wave is done with K(c)
    if (more) gload(Kh, a.ldk, c + 1, 0, false);  // K(c + 1) travels under the softmax and the second product
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
      const float f = expf(m - mn);
      float ps = 0.f;
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = expf(__builtin_fmaf(S(sb)[r], a.scale, -mn));
          ps += p;
          if (DROP) S(sb)[r] = dropout_keep(a.seed, a.site, as_drop_idx(prow, a.heads, h, c * AS_KT + 32 * sb + as_crow(r, lh)), a.thr) ? p * a.keep_scale : 0.f;
          else S(sb)[r] = p;
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      l = l * f + ps;
      m = mn;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] *= f;
      as_accum<NB>(Vimg, 0, li, lh, s0, o);
    }
    if (more) { swrite(Kimg, 0); gload(Kh, a.ldk, c + 1, 1, false); }
    if (live) as_accum<NB>(Vimg, 1, li, lh, s1, o);
    if (more) swrite(Kimg, 1);
  }

  if (!live) return;
  const float lt = l + __shfl_xor(l, 32);
  const int q = w.r0 + w.li;
  if (q >= T) return;
  as_store_row<NB, true>(w, dh, a.ctx, a.ldc, o, lt);
  if (a.lse && lh == 0) a.lse[(d.row0 + q) * (int64_t)a.heads + h] = m + logf(lt);
  if (a.ml && lh == 0) a.ml[(d.row0 + q) * (int64_t)a.heads + h] = make_float2(m, lt);
}

template <int NB> constexpr int AS_LDS = 2 * AsGeom<NB>::IMG * 4;
}  // namespace

size_t attn_stream_ws_bytes(int n_seq) { return align_up((size_t)n_seq * sizeof(AsSeq), 256); }

int attn_stream_check(int D, int heads, int n_seq, const int32_t* off, int64_t* strips) {
  SUMK_ARG(D > 0 && heads > 0 && D % heads == 0, "attn_stream: D=%d is not a positive multiple of n_heads=%d", D, heads);
  const int dh = D / heads;
  SUMK_ARG(dh % 4 == 0 && dh <= AS_MAX_DH, "attn_stream: head width %d (D=%d, n_heads=%d) must be a multiple of 4, at most %d", dh, D, heads, AS_MAX_DH);
  SUMK_ARG(n_seq > 0 && n_seq <= AS_MAX_SEQ && off && off[0] == 0, "attn_stream: n_seq=%d (1 .. %d videos, seq_off[0] == 0)", n_seq, AS_MAX_SEQ);
  int64_t n = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int T = off[s + 1] - off[s];
    SUMK_ARG(T > 0, "attn_stream: video %d has %d frames", s, T);
    SUMK_ARG(T < AS_MAX_T, "attn_stream: video %d has %d frames (limit 2^20)", s, T);
    n += (T + AS_QS - 1) / AS_QS;
  }
  SUMK_ARG(n * heads < ((int64_t)1 << 31), "attn_stream: %lld workgroups", (long long)(n * heads));
  if (strips) *strips = n;
  return SUMK_OK;
}

void attn_stream_setup(const int32_t* off_dev, int n_seq, void* ws, hipStream_t stream) {
  hipLaunchKernelGGL(as_setup_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, stream, off_dev, n_seq, (AsSeq*)ws);
}

// tag: the profiler tag of the attention launch; ml / dl / site: the training form (ml null and dl.thr == 0: the inference call)
static int as_run(const char* who, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int D, int heads, int n_seq,
                  const int32_t* off_host, const int32_t* off_dev, float scale, float* ctx, int ldc, float* lse, float2* ml, Drop dl,
                  uint32_t site, void* ws, int tag, hipStream_t stream) {
  SUMK_ARG(Q && K && V && ctx && off_dev && ws, "%s: null pointer", who);
  int64_t strips;
  SUMK_TRY(attn_stream_check(D, heads, n_seq, off_host, &strips));
  SUMK_ARG(ldq >= D && ldk >= D && ldv >= D && ldc >= D, "%s: leading dimensions (%d, %d, %d, %d) must be at least D=%d", who, ldq, ldk, ldv, ldc, D);
  SUMK_ARG(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldc % 4 == 0, "%s: leading dimensions (%d, %d, %d, %d) must be multiples of 4", who, ldq, ldk, ldv, ldc);
  SUMK_TRY(as_check_operands(who, (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)ctx, "Q, K, V and ctx", scale));
  AsArgs a;
  a.Q = Q; a.K = K; a.V = V; a.ctx = ctx; a.lse = lse; a.seq = (const AsSeq*)ws;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldc = ldc; a.dh = D / heads; a.heads = heads; a.n_seq = n_seq; a.scale = scale;
  a.ml = ml; a.seed = dl.seed; a.site = site; a.thr = dl.thr; a.keep_scale = dl.scale;
  attn_stream_setup(off_dev, n_seq, ws, stream);
  const unsigned blocks = (unsigned)(strips * heads);
  prof_begin(tag, stream);
  SUMK_TRY(as_dispatch<8>(a.dh, dl.thr != 0, [&](auto nb, auto drop) {
    return as_launch<as_stream_kernel<nb(), drop()>>(a, blocks, AS_LDS<nb()>, stream);
  }));
  prof_end(tag, stream);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

int launch_attn_stream(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int D, int heads, int n_seq,
                       const int32_t* off_host, const int32_t* off_dev, float scale, float* ctx, int ldc, float* lse, void* ws,
                       hipStream_t stream) {
  return as_run("attn_stream", Q, ldq, K, ldk, V, ldv, D, heads, n_seq, off_host, off_dev, scale, ctx, ldc, lse, nullptr, make_drop(0.f, 0), 0u, ws,
                SUMK_PROF_ATTN_STREAM, stream);
}

int launch_attn_stream_train(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int D, int heads, int n_seq,
                             const int32_t* off_host, const int32_t* off_dev, float scale, Drop dl, uint32_t site, float* ctx, int ldc,
                             float* stats, void* ws, hipStream_t stream) {
  SUMK_ARG(stats && ((uintptr_t)stats & 7) == 0, "attn_stream_train: stats must be a non-null, 8-byte aligned (n_rows, n_heads, 2) array");
  SUMK_ARG(!dl.seed_dev, "attn_stream_train: no device seed word");
  return as_run("attn_stream_train", Q, ldq, K, ldk, V, ldv, D, heads, n_seq, off_host, off_dev, scale, ctx, ldc, nullptr, (float2*)stats, dl, site,
                ws, SUMK_PROF_ATTN_STREAM_TRAIN, stream);
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_attn_stream_workspace_bytes(int32_t D, int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host) {
  if (attn_stream_check(D, n_heads, n_seq, seq_off_host) != SUMK_OK) return 0;
  return attn_stream_ws_bytes(n_seq);
}

extern "C" int sumk_attn_stream(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                                int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                                float* ctx, int32_t ldc, float* lse, void* workspace, size_t workspace_bytes, void* stream) {
  SUMK_ARG(workspace, "attn_stream: null pointer");
  SUMK_TRY(attn_stream_check(D, n_heads, n_seq, seq_off_host));
  const size_t need = attn_stream_ws_bytes(n_seq);
  if (workspace_bytes < need) { set_error("attn_stream: workspace %zu < required %zu", workspace_bytes, need); return SUMK_ERR_WORKSPACE; }
  return launch_attn_stream(Q, ldq, K, ldk, V, ldv, D, n_heads, n_seq, seq_off_host, seq_off_dev, scale, ctx, ldc, lse, workspace,
                            (hipStream_t)stream);
}

extern "C" int sumk_attn_stream_train(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                                      int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                                      float dropout_p, uint64_t seed, uint32_t site, float* ctx, int32_t ldc, float* stats, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  SUMK_ARG(workspace, "attn_stream_train: null pointer");
  SUMK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "attn_stream_train: dropout_p=%g must lie in [0, 1)", (double)dropout_p);
  SUMK_TRY(attn_stream_check(D, n_heads, n_seq, seq_off_host));
  const size_t need = attn_stream_ws_bytes(n_seq);
  if (workspace_bytes < need) { set_error("attn_stream_train: workspace %zu < required %zu", workspace_bytes, need); return SUMK_ERR_WORKSPACE; }
  return launch_attn_stream_train(Q, ldq, K, ldk, V, ldv, D, n_heads, n_seq, seq_off_host, seq_off_dev, scale, make_drop(dropout_p, seed), site,
                                  ctx, ldc, stats, workspace, (hipStream_t)stream);
}
