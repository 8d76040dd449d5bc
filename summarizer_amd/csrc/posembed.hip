// Positional embeddings for PACKED batches (vasnet.py:106-112, transformer.py:82-88 with batch size 1 per video): row off[v] + t of the
// batch gets table[t].  Out of place -- x is a dataset tensor shared by every epoch -- and straight into the forms the packed pipeline
// reads: fp32, bf16 (the mixed-precision step's shadow of x) and KB planes (the split-bf16 scoring GEMMs' operand), so the pipeline
// behind the add runs as for a model without positions.  The table's gradient is the matching gather: one thread per (t, 4 columns)
// adds the videos in ascending order -- no atomics, one fixed summation order.
#include "sumk_internal.h"
#include "pw_common.h"
#include <algorithm>

namespace sumk {

typedef unsigned int u32x4p __attribute__((ext_vector_type(4)));

// One block: 64 rows x 128 columns, the block shape of split_planes_kernel (gemm_pw.hip).  The first wave finds each row's position by a
// binary search of the sequence offsets; rows are then read coalesced (512-byte row segments, 16 bytes per lane) from x and the table,
// the sum leaves as fp32 / bf16 from registers and -- NP > 0 -- goes through LDS so that lane = row writes, per 8-column chunk and
// plane, the 16-byte chunk of its row: 64 lanes = 1 KiB contiguous of one sub-array.  Rows in [R, pitch) of the planes are zeros.
template <int NP>
__global__ __launch_bounds__(256) void pos_add_packed_kernel(const float* __restrict__ x, const float* __restrict__ table, const int32_t* __restrict__ off,
                                                             int n_seq, int64_t R, int D, int table_rows, float* __restrict__ y32,
                                                             unsigned short* __restrict__ y16, char* __restrict__ planes, int64_t rp16) {
  __shared__ float tile[NP > 0 ? 64 : 1][132];
  __shared__ int spos[64];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int c0 = blockIdx.y * 128;
  if (tid < 64) {
    const int64_t r = r0 + tid;
    int pos = 0;
    if (r < R) {
      int lo = 0, hi = n_seq;                       // largest v with off[v] <= r
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= r) lo = mid; else hi = mid;
      }
      pos = (int)(r - off[lo]);
      pos = min(max(pos, 0), table_rows - 1);       // (the host refused longer videos; device offsets that disagree must still not read past the table)
    }
    spos[tid] = pos;
  }
  __syncthreads();
  const bool pair16 = (D & 7) == 0;                 // bf16 rows start on 16-byte boundaries: an even lane stores its neighbour's four values too
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = tid + 256 * j, r = i >> 5, c4 = (i & 31) * 4;
    const bool ok = r0 + r < R && c0 + c4 < D;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
      const float4 a = *reinterpret_cast<const float4*>(x + (r0 + r) * D + c0 + c4);
      const float4 b = *reinterpret_cast<const float4*>(table + (int64_t)spos[r] * D + c0 + c4);
      v = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
      if (y32) *reinterpret_cast<float4*>(y32 + (r0 + r) * D + c0 + c4) = v;
    }
    if (y16) {                                      // (uniform: every lane takes part in the exchange)
      const u32x2 mine = __builtin_bit_cast(u32x2, __builtin_convertvector(f32x4{v.x, v.y, v.z, v.w}, bf16x4));
      const unsigned ox = __shfl_down(mine.x, 1), oy = __shfl_down(mine.y, 1);
      unsigned short* const dst = y16 + (r0 + r) * D + c0 + c4;
      if (ok && pair16) {
        if ((tid & 1) == 0) {
          if (c0 + c4 + 4 < D) *reinterpret_cast<u32x4p*>(dst) = u32x4p{mine.x, mine.y, ox, oy};
          else *reinterpret_cast<u32x2*>(dst) = mine;
        }
      } else if (ok) {
        *reinterpret_cast<u32x2*>(dst) = mine;
      }
    }
    if (NP > 0) *reinterpret_cast<float4*>(&tile[NP > 0 ? r : 0][c4]) = v;
  }
  if (NP > 0) {
    __syncthreads();
    const int r = tid & 63, cg = tid >> 6;          // 4 chunk groups x 4 chunks of 8 columns
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ch = cg * 4 + q, k = c0 + ch * 8;
      if (k >= D) continue;
      const float4 lo = *reinterpret_cast<const float4*>(&tile[NP > 0 ? r : 0][ch * 8]), hi = *reinterpret_cast<const float4*>(&tile[NP > 0 ? r : 0][ch * 8 + 4]);
      u32x2 pa[NP > 0 ? NP : 1], pb[NP > 0 ? NP : 1];
      split4<(NP > 0 ? NP : 1)>(f32x4{lo.x, lo.y, lo.z, lo.w}, pa);
      split4<(NP > 0 ? NP : 1)>(f32x4{hi.x, hi.y, hi.z, hi.w}, pb);
      char* const op = planes + ((int64_t)((k >> 4) * NP) * 2 + ((k >> 3) & 1)) * rp16 + (r0 + r) * 16;
#pragma unroll
      for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x4p*>(op + (int64_t)p * 2 * rp16) = u32x4p{pa[p].x, pa[p].y, pb[p].x, pb[p].y};
    }
  }
}

// dtable[t, c .. c + 3] += sum over the videos with len > t of dx[off[v] + t, c .. c + 3]: thread = (t, column chunk), videos in ascending
// order, plain fp32 adds starting from the value dtable holds.  Consecutive lanes own consecutive 16-byte chunks of a row.
__global__ __launch_bounds__(256) void pos_table_grad_kernel(const float* __restrict__ dx, const int32_t* __restrict__ off, int n_seq, int D, int t_max,
                                                             float* __restrict__ dtable) {
  const int d4 = D >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)t_max * d4) return;
  const int t = (int)(i / d4), c = (int)(i % d4) * 4;
  float4 acc = *reinterpret_cast<const float4*>(dtable + (int64_t)t * D + c);
  int o0 = off[0];
  for (int v = 0; v < n_seq; ++v) {
    const int o1 = off[v + 1];
    if (o1 - o0 > t) {
      const float4 g = *reinterpret_cast<const float4*>(dx + ((int64_t)o0 + t) * D + c);
      acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
    }
    o0 = o1;
  }
  *reinterpret_cast<float4*>(dtable + (int64_t)t * D + c) = acc;
}

// longest video of the batch, or -1 when the host offsets do not describe one (not starting at 0, an empty or negative-length video)
static int longest_video(int32_t n_seq, const int32_t* seq_off_host) {
  if (n_seq < 1 || !seq_off_host || seq_off_host[0] != 0) return -1;
  int t_max = 0;
  for (int v = 0; v < n_seq; ++v) {
    const int len = seq_off_host[v + 1] - seq_off_host[v];
    if (len < 1) return -1;
    t_max = std::max(t_max, len);
  }
  return t_max;
}

}  // namespace sumk

using namespace sumk;

extern "C" int sumk_pos_add_packed(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                   const float* table, int32_t table_rows, float* out_f32, void* out_bf16, void* out_planes,
                                   int32_t n_planes, void* stream) {
  SUMK_ARG(x && seq_off_host && seq_off_dev && table && D >= 4 && table_rows >= 1, "pos_add_packed: null pointer or empty shape");
  SUMK_ARG(out_f32 || out_bf16 || out_planes, "pos_add_packed: no output asked for");
  SUMK_ARG(D % 4 == 0, "pos_add_packed: D=%d is not a multiple of 4", D);
  const int t_max = longest_video(n_seq, seq_off_host);
  SUMK_ARG(t_max >= 1, "pos_add_packed: bad sequence offsets");
  SUMK_ARG(t_max <= table_rows, "pos_add_packed: input sequence has higher length (%d) than max_length (%d)", t_max, table_rows);
  SUMK_ARG(!out_planes || ((n_planes == 2 || n_planes == 3) && D % 16 == 0), "pos_add_packed: planes need D %% 16 == 0 and 2 or 3 planes (D=%d, planes=%d)", D, n_planes);
  SUMK_ARG((((uintptr_t)x | (uintptr_t)table | (uintptr_t)out_f32 | (uintptr_t)out_planes) & 15) == 0 && ((uintptr_t)out_bf16 & (D % 8 == 0 ? 15 : 7)) == 0,
           "pos_add_packed: 16-byte aligned buffers");
  const int64_t R = seq_off_host[n_seq];
  const int64_t rp = pw_rows_pitch(R);
  const dim3 grid((unsigned)(rp / 64), (unsigned)((D + 127) / 128));
  const int np = out_planes ? n_planes : 0;
#define SUMK_POS_LAUNCH(NP)                                                                                                              \
  hipLaunchKernelGGL(pos_add_packed_kernel<NP>, grid, dim3(256), 0, (hipStream_t)stream, x, table, seq_off_dev, n_seq, R, D, table_rows, \
                     out_f32, (unsigned short*)out_bf16, (char*)out_planes, rp * 16)
  if (np == 3) SUMK_POS_LAUNCH(3);
  else if (np == 2) SUMK_POS_LAUNCH(2);
  else SUMK_POS_LAUNCH(0);
#undef SUMK_POS_LAUNCH
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}

extern "C" int sumk_pos_table_grad(const float* dx, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                   float* dtable, int32_t table_rows, void* stream) {
  SUMK_ARG(dx && seq_off_host && seq_off_dev && dtable && D >= 4 && D % 4 == 0 && table_rows >= 1, "pos_table_grad: null pointer or bad shape (D %% 4)");
  const int t_max = longest_video(n_seq, seq_off_host);
  SUMK_ARG(t_max >= 1, "pos_table_grad: bad sequence offsets");
  SUMK_ARG(t_max <= table_rows, "pos_table_grad: input sequence has higher length (%d) than max_length (%d)", t_max, table_rows);
  SUMK_ARG((((uintptr_t)dx | (uintptr_t)dtable) & 15) == 0, "pos_table_grad: 16-byte aligned buffers");
  const int64_t n = (int64_t)t_max * (D >> 2);
  hipLaunchKernelGGL(pos_table_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, seq_off_dev, n_seq, D, t_max, dtable);
  SUMK_HIP(hipGetLastError());
  return SUMK_OK;
}
