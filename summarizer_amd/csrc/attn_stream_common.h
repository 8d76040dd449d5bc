// What the streaming attention units share (attn_stream.hip: forward; attn_stream_bwd.hip: backward): the tile geometry, the per-video
// descriptor and the lane maps of the v_mfma_f32_32x32x2_f32 accumulator.
#pragma once
#include "gemm_device.h"

namespace sumk {

constexpr int AS_KT = 64;                 // rows of a walked tile (keys in the forward and the dQ pass, queries in the dK / dV pass)
constexpr int AS_QS = 128;                // rows per strip a workgroup owns: 4 waves x 32
constexpr int AS_MAX_T = 1 << 20;
constexpr int AS_MAX_SEQ = 65535;

struct AsSeq { int64_t row0; int32_t T; int32_t strip0; };   // first packed row, frames, first strip of the video

// row of accumulator register r inside a 32 x 32 block for lane half lh
__device__ __forceinline__ int as_crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

template <int W> struct AsVec;
template <> struct AsVec<1> { float v[1]; __device__ __forceinline__ void load(const float* p) { v[0] = *p; } };
template <> struct AsVec<2> { float v[2]; __device__ __forceinline__ void load(const float* p) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; } };
template <> struct AsVec<4> { float v[4]; __device__ __forceinline__ void load(const float* p) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; } };

// index of the dropout mask of weight (packed query row, head, key): the one tf_softmax_kernel (transformer.hip) uses
__device__ __forceinline__ uint64_t as_drop_idx(int64_t packed_row, int heads, int h, int key) {
  return ((uint64_t)(packed_row * heads + h) << 20) | (uint64_t)key;
}

// the per-video descriptors (attn_stream_ws_bytes(n_seq) bytes at `ws`) both units' kernels read; strips of AS_QS rows
void attn_stream_setup(const int32_t* off_dev, int n_seq, void* ws, hipStream_t stream);

}  // namespace sumk
