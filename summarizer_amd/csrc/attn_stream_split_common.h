// What the bf16x3 streaming attention units share (attn_stream_split.hip: scoring and training forward; attn_stream_split_bwd.hip:
// backward): the per-video descriptor with its padded rows, the order of a tile's rows in a TRANSPOSED plane, the batch's limits.
//
// Planes (hi = bf16(x) to nearest even, lo = bf16(x - hi); videos padded to whole 64-row tiles, head widths to DP = 32 NB columns; every
// padded row and column is written as zeros):
//   row-major    [head][padded row][hi DP | lo DP]: a 64-row tile is ONE contiguous block of 256 DP bytes.  A operand of a first product
//                (one ds_read_b128 per plane at [row][16 g + 8 lh]) and, for the owner strip, its B operand.
//   transposed   [head][tile][d][hi 64 rows | lo 64 rows], the rows of a tile in the order the accumulating product's B operand has them:
//                registers 8 s .. 8 s + 7 of a first product's accumulator, converted to bf16, ARE the B fragment of k-step s, and element
//                j of lane half lh is tile row 16 s + 8 (j >> 2) + 4 lh + (j & 3); so position p holds row p with bits 2 and 3 swapped,
//                and the A fragment is one ds_read_b128 per plane at [d][32 sb + 16 s + 8 lh].
#pragma once
#include "attn_stream_common.h"
#include "pw_common.h"

namespace sumk {

namespace {
constexpr int ASS_MAX_DH = 128;
constexpr int ASS_VP = 272;                     // bytes of a transposed image row: 64 rows x 2 planes x 2 bytes + 16

struct AssSeq { int64_t row0; int64_t prow0; int32_t T; int32_t strip0; };   // first packed row, first padded row, frames, first strip

typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// position p of a tile's 64 rows in a transposed plane <-> row: bits 2 and 3 swapped (an involution)
__device__ __forceinline__ int ass_perm(int p) { return (p & ~12) | ((p & 8) >> 1) | ((p & 4) << 1); }

__device__ __forceinline__ AssSeq ass_find(const AssSeq* seq, int n_seq, int64_t key, bool by_strip) {
  int lo = 0, hi = n_seq - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const int64_t v = by_strip ? (int64_t)seq[mid].strip0 : seq[mid].prow0;
    if (v <= key) lo = mid; else hi = mid - 1;
  }
  return seq[lo];
}

__global__ void ass_setup_kernel(const int32_t* off, int n_seq, AssSeq* seq) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  int strip0 = 0; int64_t prow0 = 0;
  for (int q = 0; q < s; ++q) {
    const int T = off[q + 1] - off[q];
    strip0 += (T + AS_QS - 1) / AS_QS;
    prow0 += (int64_t)((T + AS_KT - 1) / AS_KT) * AS_KT;
  }
  AssSeq d; d.row0 = off[s]; d.prow0 = prow0; d.T = off[s + 1] - off[s]; d.strip0 = strip0;
  seq[s] = d;
}

__device__ __forceinline__ bf16x8 ass_ld(const char* p) { return *reinterpret_cast<const bf16x8*>(p); }

// the batch's limits for the bf16x3 units; *rp: padded rows (a multiple of 64), *strips: strips of 128 rows, *nb: staged width / 32
inline int ass_check(const char* who, int D, int heads, int n_seq, const int32_t* off, int precision, int64_t* rp_out, int64_t* strips, int* nb) {
  SUMK_ARG(precision == SUMK_PRECISION_BF16X3, "%s: precision=%d (only SUMK_PRECISION_BF16X3 = %d)", who, precision, SUMK_PRECISION_BF16X3);
  SUMK_ARG(D > 0 && heads > 0 && D % heads == 0, "%s: D=%d is not a positive multiple of n_heads=%d", who, D, heads);
  const int dh = D / heads;
  SUMK_ARG(dh % 8 == 0 && dh <= ASS_MAX_DH, "%s: head width %d (D=%d, n_heads=%d) must be a multiple of 8, at most %d", who, dh, D, heads, ASS_MAX_DH);
  SUMK_ARG(n_seq > 0 && n_seq <= AS_MAX_SEQ && off && off[0] == 0, "%s: n_seq=%d (1 .. %d videos, seq_off[0] == 0)", who, n_seq, AS_MAX_SEQ);
  int64_t n = 0, rp = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int T = off[s + 1] - off[s];
    SUMK_ARG(T > 0, "%s: video %d has %d frames", who, s, T);
    SUMK_ARG(T < AS_MAX_T, "%s: video %d has %d frames (limit 2^20)", who, s, T);
    n += (T + AS_QS - 1) / AS_QS;
    rp += (int64_t)((T + AS_KT - 1) / AS_KT) * AS_KT;
  }
  SUMK_ARG(n * heads < ((int64_t)1 << 31) && rp / AS_KT < ((int64_t)1 << 31), "%s: %lld workgroups", who, (long long)(n * heads));
  *nb = dh <= 32 ? 1 : dh <= 64 ? 2 : 4;
  *rp_out = rp; *strips = n;
  return SUMK_OK;
}
}  // namespace

}  // namespace sumk
