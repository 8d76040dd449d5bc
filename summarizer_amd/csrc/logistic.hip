// The logistic-regression baseline's training step in ONE launch (summarizer/models/logistic.py:67-88: per-video nn.MSELoss of
// sigmoid(x w + b) against the min-max normalised gtscore, backward, torch.optim.Adam(lr, weight_decay) step).  As torch runs it that
// is a GEMV, the sigmoid, the MSE, their backward passes, a reduction per parameter tensor and the Adam kernels -- several small
// launches for 1 025 parameters -- plus a float(loss) host sync per video.  Here:
//
//   pass 1, every block: a contiguous range of rows of the packed batch.  A wave holds a row (D/64 floats per lane: 16 at D = 1024,
//     two rows in flight per wave), reduces x.w, applies the sigmoid, and accumulates g x into per-lane registers, where
//       g_r = 2 (s_r - t_r) / T_v * scale * s_r (1 - s_r)     (the composition segment_mse_mean backward -> frame-head backward),
//     and stores the row's squared error e_r = (s_r - t_r)^2 (and, optionally, its score).  The block's four waves are added in wave
//     order through LDS and the block writes its D + 4 partials [dW (D) | db, 0, 0, 0] to its workspace slab.
//   hand-off (cdna_hip_programming.md section 6, Guideline 16, sc1 form -- the SK path of gemm_lean.hip): every handed-off byte (slabs
//     and e_r) is stored write-through (sc1), every storing wave drains vmcnt(0), workgroup barrier, ONE relaxed agent-scope ticket add;
//     the last arriver reads those bytes with sc1 loads ONLY, so no fence is needed and nothing depends on block placement.
//   pass 2, the last arriver: adds the slabs in BLOCK-INDEX order (never in arrival order: the result is bit-deterministic), computes
//     mse[v] = sum_t e / T_v per video and loss = scale * sum_v mse[v] in video order (the step loss of sumk_segment_mse_mean_forward),
//     then EITHER applies torch's Adam to [w | b] with the bias corrections of the device step counter (the arithmetic of
//     sumk_adam_step_dev, counter incremented) OR adds [dW | db] to the gradient bucket (.grad semantics; the data-parallel path
//     all-reduces it and runs FlatAdam.step()).
//
// Grid: G = min(ceil(R / 32), ceil(sqrt(R)), 256) blocks for R rows.  The first pass costs about R / G dependent row loads per block,
// the serial part of the second about G slab rows (D + 4 floats each) for the one reducing block, so the sum is smallest near
// G = sqrt(R); below R = 1024 the 32-rows-per-block floor wins (a block that reads fewer rows than that is all launch and hand-off).
// One T = 300 video: 10 blocks, 40 KB of slabs at D = 1024; 50 videos (~12 000 rows): 110 blocks, 450 KB, where one block per
// 32 rows would leave 1.5 MB for the reducer.  First measurement (MI355X, D = 1024, CUDA-event timing of back-to-back steps, memset
// included): 16.0 us per step at 240 rows, 16.4 us at 300, 64 us at 50 x 240 rows; the kernel alone 12-15 us per step in a kernel
// trace of trainer epochs (150-320 rows).  No target is claimed: the first pass is latency-bound at these sizes.
//
// Workspace: [ticket word, in a 16-byte block of its own at the start][G slabs of D + 4 floats][e: R floats].  The launch function
// zeroes the 16-byte block with hipMemsetAsync on every call (Guideline 16, "Re-initialise every call": a captured step replays the
// memset node, and the first launch on a poisoned workspace is valid); the last arriver also leaves the word zero, so a memset node
// that bypasses the L2 line the previous replay's atomics left behind (the finding behind lstm.hip's zero_words_kernel) still finds 0.
#include "sumk_internal.h"
#include <math.h>
#include <algorithm>

namespace sumk {

typedef unsigned int lg_u32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int LG_THREADS = 256;
constexpr int LG_MAX_D = 2048;               // NV = 8 float4 per lane
constexpr int LG_MAX_BLOCKS = 256;
constexpr int LG_RSRC_FLAGS = 0x00020000;    // buffer descriptor word 3 (as gemm_lean.hip)

int lg_blocks(int n_rows) {
  const int by_rows = (n_rows + 31) / 32;
  const int by_sqrt = (int)ceil(sqrt((double)n_rows));
  return std::max(1, std::min(std::min(by_rows, by_sqrt), LG_MAX_BLOCKS));
}

struct LgWs { size_t slab, err, total; };
LgWs lg_carve(int n_rows, int D) {
  LgWs w;
  w.slab = 256;                                                     // [0, 16): the ticket block; the rest of the first 256 B unused
  w.err = align_up(w.slab + (size_t)lg_blocks(n_rows) * (D + 4) * 4, 256);
  w.total = align_up(w.err + (size_t)n_rows * 4, 256);
  return w;
}

struct LgArgs {
  const float* x; const float* target; const int32_t* off; int32_t n_seq, n_rows, D;
  float* param; float* grad; float* m; float* v; int32_t* state;
  float lr, b1, b2, omb1, omb2, eps, wd, scale, grad_scale;   // omb = 1 - beta, taken in double (optim.hip)
  double b1d, b2d;
  float* loss; float* mse; float* scores;
  unsigned* ticket; float* slab; float* err;
  int32_t apply_adam;
};

__device__ __forceinline__ float4 lg_as4(lg_u32x4 v) { return __builtin_bit_cast(float4, v); }
__device__ __forceinline__ lg_u32x4 lg_asu(float4 v) { return __builtin_bit_cast(lg_u32x4, v); }
}  // namespace

template <int NV>
__global__ __launch_bounds__(LG_THREADS) void logistic_step_kernel(LgArgs a) {
  constexpr int WSLOT = NV * 256 + 4;                  // floats of one wave's partial row in LDS (>= D + 4)
  __shared__ float lds[4 * WSLOT + 4];                 // ONE __shared__ object: wave partials, per-video values, the ticket broadcast
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = a.D, S4 = (D >> 2) + 1;                // float4s of a slab row: [w (D) | b, 0, 0, 0]
  const int G = gridDim.x;
  const int lo = (int)((int64_t)blockIdx.x * a.n_rows / G), hi = (int)((int64_t)(blockIdx.x + 1) * a.n_rows / G);

  // ---- pass 1: rows [lo, hi) of this block, wave w takes rows lo + w, lo + w + 4, ... (two in flight)
  // Out-of-range columns (lanes past D / 4) read zeros through the descriptors' record limit: no per-load predicate.
  const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(a.param, (short)0, D * 4, LG_RSRC_FLAGS);
  float4 w[NV], acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    w[j] = lg_as4(__builtin_amdgcn_raw_buffer_load_b128(rW, (lane + 64 * j) * 16, 0, 0));
    acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float bias = a.param[D];
  float accb = 0.f;
  int v = 0;
  {                                                    // the video of the block's first row (wave-uniform binary search)
    int l = 0, h = a.n_seq - 1;
    while (l < h) { const int mid = (l + h) >> 1; if (a.off[mid + 1] <= lo) l = mid + 1; else h = mid; }
    v = l;
  }
  const __amdgpu_buffer_rsrc_t rE = __builtin_amdgcn_make_buffer_rsrc(a.err, (short)0, a.n_rows * 4, LG_RSRC_FLAGS);
  for (int r = lo + wave; r < hi; r += 8) {
    const bool two = r + 4 < hi;                       // wave-uniform
    int va = v;
    while (a.off[va + 1] <= r) ++va;
    int vb = va;
    if (two) while (a.off[vb + 1] <= r + 4) ++vb;
    v = vb;
    const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x) + (int64_t)r * D, (short)0, D * 4, LG_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x) + (int64_t)(two ? r + 4 : r) * D, (short)0,
                                                                        two ? D * 4 : 0, LG_RSRC_FLAGS);
    float4 xa[NV], xb[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      xa[j] = lg_as4(__builtin_amdgcn_raw_buffer_load_b128(rA, (lane + 64 * j) * 16, 0, 0));
      xb[j] = lg_as4(__builtin_amdgcn_raw_buffer_load_b128(rB, (lane + 64 * j) * 16, 0, 0));
    }
    float da = 0.f, db = 0.f;                          // the frame head's order: pairs, then columns ascending, then the lanes
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      da += (xa[j].x * w[j].x + xa[j].y * w[j].y) + (xa[j].z * w[j].z + xa[j].w * w[j].w);
      db += (xb[j].x * w[j].x + xb[j].y * w[j].y) + (xb[j].z * w[j].z + xb[j].w * w[j].w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { da += __shfl_xor(da, o); db += __shfl_xor(db, o); }
    const float sa = 1.0f / (1.0f + expf(-(da + bias))), sb = 1.0f / (1.0f + expf(-(db + bias)));
    const float ta = a.target[r], tb = a.target[two ? r + 4 : r];
    const float ea = sa - ta, eb = sb - tb;
    // dscores = 2 (dloss * scale) / T * (s - t) with dloss = 1 (segment_mse_mean_bwd_kernel), then * s (1 - s) (frame_head_bwd_kernel)
    const float ga = ((2.f * a.scale / (float)(a.off[va + 1] - a.off[va])) * ea) * sa * (1.f - sa);
    const float gb = two ? ((2.f * a.scale / (float)(a.off[vb + 1] - a.off[vb])) * eb) * sb * (1.f - sb) : 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      acc[j].x += ga * xa[j].x; acc[j].y += ga * xa[j].y; acc[j].z += ga * xa[j].z; acc[j].w += ga * xa[j].w;
      acc[j].x += gb * xb[j].x; acc[j].y += gb * xb[j].y; acc[j].z += gb * xb[j].z; acc[j].w += gb * xb[j].w;
    }
    accb += ga; accb += gb;
    if (lane == 0) {
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ea * ea), rE, r * 4, 0, 16 /* sc1 */);
      if (two) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, eb * eb), rE, (r + 4) * 4, 0, 16 /* sc1 */);
      if (a.scores) { a.scores[r] = sa; if (two) a.scores[r + 4] = sb; }
    }
  }

  // ---- the block's partial: the four waves added in wave order, stored write-through to slab[blockIdx.x]
  float* mine = lds + wave * WSLOT;
#pragma unroll
  for (int j = 0; j < NV; ++j) reinterpret_cast<float4*>(mine)[lane + 64 * j] = acc[j];
  if (lane == 0) reinterpret_cast<float4*>(mine)[D >> 2] = make_float4(accb, 0.f, 0.f, 0.f);   // (after the zeros of column D/4: LDS is in order per wave)
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(a.slab, (short)0, G * S4 * 16, LG_RSRC_FLAGS);
  for (int c = tid; c < S4; c += LG_THREADS) {
    const float4 p0 = reinterpret_cast<const float4*>(lds)[c], p1 = reinterpret_cast<const float4*>(lds + WSLOT)[c];
    const float4 p2 = reinterpret_cast<const float4*>(lds + 2 * WSLOT)[c], p3 = reinterpret_cast<const float4*>(lds + 3 * WSLOT)[c];
    const float4 s = make_float4(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y, ((p0.z + p1.z) + p2.z) + p3.z,
                                 ((p0.w + p1.w) + p2.w) + p3.w);
    __builtin_amdgcn_raw_buffer_store_b128(lg_asu(s), rS, ((int)blockIdx.x * S4 + c) * 16, 0, 16 /* sc1 */);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // EVERY storing wave drains its write-through stores (slab and e)
  __syncthreads();
  int* flag = reinterpret_cast<int*>(lds + 4 * WSLOT);
  if (tid == 0) *flag = (int)__hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (*flag != G - 1) return;

  // ---- pass 2, the last arriver.  Every load of handed-off bytes below is an sc1 load.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // no instruction: keeps the compiler from hoisting the loads
  float step_size = 0.f, inv_sqrt_bc2 = 0.f;
  if (a.apply_adam) {
    // adam_prep_kernel's arithmetic (optim.hip), counter and scratch words included; broadcast through LDS
    __syncthreads();                                   // (every thread has read *flag before the slot is reused)
    if (tid == 0) {
      const int step = a.state[0] + 1;
      a.state[0] = step;
      const double bc1 = 1.0 - pow(a.b1d, (double)step);
      const double bc2 = 1.0 - pow(a.b2d, (double)step);
      float* f = reinterpret_cast<float*>(a.state);
      f[1] = (float)((double)a.lr / bc1);
      f[2] = (float)(1.0 / sqrt(bc2));
      f[3] = (float)(double)a.grad_scale;
      lds[4 * WSLOT] = f[1]; lds[4 * WSLOT + 1] = f[2];
    }
    __syncthreads();
    step_size = lds[4 * WSLOT]; inv_sqrt_bc2 = lds[4 * WSLOT + 1];
  }
  for (int c = tid; c < S4; c += LG_THREADS) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    int b = 0;
    for (; b + 4 <= G; b += 4) {                       // four slabs in flight, added in block order
      float4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = lg_as4(__builtin_amdgcn_raw_buffer_load_b128(rS, ((b + u) * S4 + c) * 16, 0, 16 /* sc1 */));
#pragma unroll
      for (int u = 0; u < 4; ++u) { g.x += q[u].x; g.y += q[u].y; g.z += q[u].z; g.w += q[u].w; }
    }
    for (; b < G; ++b) {
      const float4 q = lg_as4(__builtin_amdgcn_raw_buffer_load_b128(rS, (b * S4 + c) * 16, 0, 16 /* sc1 */));
      g.x += q.x; g.y += q.y; g.z += q.z; g.w += q.w;
    }
    if (!a.apply_adam) {                               // .grad semantics: accumulate
      float4 gg = reinterpret_cast<const float4*>(a.grad)[c];
      gg.x += g.x; gg.y += g.y; gg.z += g.z; gg.w += g.w;
      reinterpret_cast<float4*>(a.grad)[c] = gg;
      continue;
    }
    // adam_kernel's update (optim.hip), the same expression per element
    float4 pp = reinterpret_cast<float4*>(a.param)[c], gg = g;
    float4 mm = reinterpret_cast<float4*>(a.m)[c], vv = reinterpret_cast<float4*>(a.v)[c];
    const float b1 = a.b1, b2 = a.b2, omb1 = a.omb1, omb2 = a.omb2, eps = a.eps, wd = a.wd, grad_scale = a.grad_scale;
#define LG_ADAM1(c)                                                     \
    {                                                                   \
      float gr = gg.c * grad_scale + wd * pp.c;                         \
      mm.c = b1 * mm.c + omb1 * gr;                                     \
      vv.c = b2 * vv.c + omb2 * gr * gr;                                \
      pp.c -= step_size * (mm.c / (sqrtf(vv.c) * inv_sqrt_bc2 + eps));  \
    }
    LG_ADAM1(x) LG_ADAM1(y) LG_ADAM1(z) LG_ADAM1(w)
#undef LG_ADAM1
    reinterpret_cast<float4*>(a.param)[c] = pp; reinterpret_cast<float4*>(a.m)[c] = mm; reinterpret_cast<float4*>(a.v)[c] = vv;
  }

  // per-video MSE (wave w: videos w, w + 4, ... of each group of 256) and the loss, added in video order by one thread
  float part = 0.f;
  for (int q0 = 0; q0 < a.n_seq; q0 += 256) {
    __syncthreads();                                   // (the previous group's values are consumed)
    const int nq = min(256, a.n_seq - q0);
    for (int i = wave; i < nq; i += 4) {
      const int r0 = a.off[q0 + i], T = a.off[q0 + i + 1] - r0;
      float s = 0.f;
      for (int t = lane; t < T; t += 64) s += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rE, (r0 + t) * 4, 0, 16 /* sc1 */));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      const float mse = s / (float)T;
      if (lane == 0) { a.mse[q0 + i] = mse; lds[i] = mse; }
    }
    __syncthreads();
    if (tid == 0) for (int i = 0; i < nq; ++i) part += lds[i];
  }
  if (tid == 0) {
    a.loss[0] = part * a.scale;
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (see the header: the memset is the contract)
  }
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_logistic_step_workspace_bytes(int32_t n_rows, int32_t D) {
  if (n_rows <= 0 || D <= 0 || D % 4 != 0 || D > LG_MAX_D) return 0;
  return lg_carve(n_rows, D).total;
}

extern "C" int sumk_logistic_step(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                  const float* target, float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq,
                                  int32_t* state, float lr, double beta1, double beta2, float eps, float weight_decay, float scale,
                                  int32_t apply_adam, float* loss, float* mse_per_video, float* scores, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(x, "logistic_step: x is null");
  SUMK_ARG(target, "logistic_step: target is null");
  SUMK_ARG(seq_off_host && seq_off_dev, "logistic_step: seq_off_host / seq_off_dev is null");
  SUMK_ARG(flat_param, "logistic_step: flat_param is null");
  SUMK_ARG(loss && mse_per_video, "logistic_step: loss / mse_per_video is null");
  SUMK_ARG(workspace, "logistic_step: workspace is null");
  SUMK_ARG(D > 0 && D % 4 == 0 && D <= LG_MAX_D, "logistic_step: bad D=%d (a multiple of 4 in [4, %d])", D, LG_MAX_D);
  SUMK_ARG(n_seq > 0, "logistic_step: bad n_seq=%d", n_seq);
  if (apply_adam) {
    SUMK_ARG(exp_avg && exp_avg_sq, "logistic_step: exp_avg / exp_avg_sq is null (fused Adam mode)");
    SUMK_ARG(state, "logistic_step: state is null (fused Adam mode)");
  } else {
    SUMK_ARG(flat_grad, "logistic_step: flat_grad is null (gradient-only mode)");
  }
  SUMK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)flat_param & 15) == 0 && ((uintptr_t)(apply_adam ? exp_avg : flat_grad) & 15) == 0 &&
           (!apply_adam || ((uintptr_t)exp_avg_sq & 15) == 0), "logistic_step: x / flat buckets must be 16-byte aligned");
  const int32_t n_rows = seq_off_host[n_seq];
  SUMK_ARG(seq_off_host[0] == 0 && n_rows > 0, "logistic_step: bad seq_off_host (n_rows=%d)", n_rows);
  for (int s = 0; s < n_seq; ++s) SUMK_ARG(seq_off_host[s + 1] > seq_off_host[s], "logistic_step: seq_off_host: empty video %d", s);
  const LgWs L = lg_carve(n_rows, D);
  if (workspace_bytes < L.total) {
    set_error("logistic_step: workspace %zu < required %zu", workspace_bytes, L.total);
    return SUMK_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  LgArgs a;
  a.x = x; a.target = target; a.off = seq_off_dev; a.n_seq = n_seq; a.n_rows = n_rows; a.D = D;
  a.param = flat_param; a.grad = flat_grad; a.m = exp_avg; a.v = exp_avg_sq; a.state = state;
  a.lr = lr; a.b1 = (float)beta1; a.b2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2); a.b1d = beta1; a.b2d = beta2; a.eps = eps; a.wd = weight_decay; a.scale = scale; a.grad_scale = 1.f;
  a.loss = loss; a.mse = mse_per_video; a.scores = scores;
  a.ticket = (unsigned*)ws; a.slab = (float*)(ws + L.slab); a.err = (float*)(ws + L.err);
  a.apply_adam = apply_adam ? 1 : 0;
  SUMK_HIP(hipMemsetAsync(ws, 0, 16, stream));        // the ticket block, every call (header)
  const int G = lg_blocks(n_rows);
  if (D <= 256) hipLaunchKernelGGL(logistic_step_kernel<1>, dim3(G), dim3(LG_THREADS), 0, stream, a);
  else if (D <= 512) hipLaunchKernelGGL(logistic_step_kernel<2>, dim3(G), dim3(LG_THREADS), 0, stream, a);
  else if (D <= 1024) hipLaunchKernelGGL(logistic_step_kernel<4>, dim3(G), dim3(LG_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(logistic_step_kernel<8>, dim3(G), dim3(LG_THREADS), 0, stream, a);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
