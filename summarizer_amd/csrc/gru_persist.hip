// Bidirectional GRU layer for a packed batch of videos on gfx950: the persistent recurrence of `DSN(cell="gru")`
// (summarizer/models/dsn.py:28-33, nn.GRU, bidirectional).  torch.nn.GRU semantics, gate order r, z, n:
//   r = sigmoid(Gx_r + Gh_r)   z = sigmoid(Gx_z + Gh_z)   n = tanh(Gx_n + r * Gh_n)   h = (1 - z) * n + z * h_prev
//   Gx = x W_ih^T + b_ih  (all frames at once: one NT GEMM per direction into G (R, 6H) = [direction][r | z | n])
//   Gh = h_prev W_hh^T + b_hh  (inside the recurrence; b_hh is added there for all three gates -- r multiplies b_hn, so it cannot
//                               move into the projection, and the other two keep it company: the sums of the step path, in its order)
// Forward and BPTT are ONE cooperative launch each per layer (H <= 256), built like lstm_persist_kernel / lstm_persist_bwd_kernel:
// 256 blocks in 8 teams of 32 (team = blockIdx % 8, for speed only), a work item = (group of <= 32 videos, direction), member m owns
// hidden units [m upm, (m + 1) upm) of every video of the item and computes r, z AND n of its units, so r * Gh_n needs no exchange.
// Every cross-block hand-off follows the placement-independent protocol written at the top of the "persistent recurrence" section of
// lstm.hip (cdna_hip_programming.md Guideline 16): the forward pass in its flag-in-data form, the BPTT in its counter form.  Every wait
// is bounded (PK_WAIT_TICKS of wall clock / PK_SPIN_LIMIT turns); a timeout sets the per-call word and g_sumk_health and the block
// stops waiting.  No float atomics: the cross-wave and cross-member sums run in a fixed order.
// H > 256 stays on the step path (gru.hip + the host loop of summarizer_amd/models/_bilstm.py).
#include "sumk_internal.h"
#include "persist_common.h"
#include <algorithm>
#include <cstdlib>

namespace sumk {

struct GruWs {
  size_t g, prob, pstate, ll, ll_bytes;                                     // inference and training
  size_t sv, hprev, dgx, dghn, slab, slab_elems, prob_sk, colpart, pstate_b, xchg, xchg_bytes;   // training only
  size_t total;
  int32_t n_rows, t_max, gsize, n_groups;
};

static int gru_carve(int In, int H, int n_seq, const int32_t* off, int training, GruWs* w) {
  SUMK_ARG(In > 0 && In % 4 == 0, "bigru: input size %d must be a positive multiple of 4", In);
  SUMK_ARG(H > 0 && H % 4 == 0 && H <= 256, "bigru: hidden size %d must be a multiple of 4 in [4, 256] (larger cells run the step path: sumk_gru_cell_forward)", H);
  SUMK_TRY(scan_sequences(n_seq, off, "bigru", "video", "frames", &w->n_rows, &w->t_max));
  const size_t R = (size_t)w->n_rows;
  SUMK_ARG(R * 2 * H * 4 < 0x7fffffffull, "bigru: %zu frames x 2H = %d exceed the 2 GB the kernels address with 32-bit offsets", R, 2 * H);
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t at = p; p += align_up(bytes, 256); return at; };
  w->gsize = pk_group_size(n_seq); w->n_groups = (n_seq + w->gsize - 1) / w->gsize;
  SUMK_ARG(pk_items_fit(2 * w->n_groups), "bigru: %d videos are more than one call takes", n_seq);
  w->g = take(R * 6 * H * 4);                        // Gx: [direction][r | z | n]
  w->prob = take(8 * sizeof(GemmProb));
  w->pstate = take(16 * 4);                          // forward: the error word alone (the hand-off carries its flags in the data)
  // flag-in-data hand-off of the forward recurrence, directly behind the state words and zeroed with them:
  // [step parity 2][direction 2][video][H] x {float h, uint32 step tag}
  w->ll_bytes = (size_t)4 * n_seq * H * 8;
  SUMK_ARG(w->ll_bytes < 0x7fffffe0ull, "bigru: %d videos are more than one call takes", n_seq);
  w->ll = take(w->ll_bytes);
  w->sv = w->hprev = w->dgx = w->dghn = w->slab = w->slab_elems = w->prob_sk = w->colpart = w->pstate_b = w->xchg = w->xchg_bytes = 0;
  if (training) {
    w->sv = take(R * 8 * H * 4);                     // r, z, n, Gh_n per row: [direction][r | z | n | Gh_n]
    w->hprev = take(R * 2 * H * 4);                  // h_{t-1} per row and direction (0 at a sequence start): the B operand of dW_hh
    w->dgx = take(R * 6 * H * 4);                    // gradient w.r.t. Gx, same layout as Gx
    w->dghn = take(R * 2 * H * 4);                   // the n block of the gradient w.r.t. Gh (its r and z blocks equal dGx's)
    const size_t big = (size_t)(6 * H) * (size_t)(In > H ? In : H);
    w->slab_elems = (size_t)8 * big;                 // split-K partial slabs of the weight gradients
    w->slab = take(w->slab_elems * 4);
    w->prob_sk = take(64 * sizeof(GemmProb));
    w->colpart = take((size_t)128 * 6 * H * 4);
    w->pstate_b = take(PSTATE_WORDS * 4);            // the BPTT's error word and step counters
    w->xchg_bytes = (size_t)2 * (2 * w->n_groups) * 32 * 32 * H * 4;   // BPTT exchange: [step parity 2][item][member 32][video 32][H] partial sums of dh
    w->xchg = take(w->xchg_bytes);
  }
  w->total = p;
  return SUMK_OK;
}

// ------------------------------------------------------------------------------------------- forward
// The member's 32 "gate columns" are n = 4 unit + gate with gate 3 EMPTY (zero weights): the tile shapes, the LDS map and the float4
// epilogue read of lstm_persist_kernel carry over unchanged, at the price of multiplying one zero column in four.
// W_hh fragments stay in registers for the whole item; h_{t-1} arrives as {value, step tag} packets and the loads are the poll.
struct GruPersistArgs {
  const float* G; const float* whh[2]; const float* bhh[2]; float* Hout;
  float* sv; float* hprev;                    // training-mode saves (nullptr in inference)
  const int32_t* off; unsigned* state; unsigned* health;
  int32_t n_seq, H, gsize, n_groups, upm, n_active;
  unsigned long long* ll; int32_t ll_bytes;
};

template <bool M16>
__global__ __launch_bounds__(PK_THREADS) void gru_persist_kernel(GruPersistArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int CPW = 4;                  // 8-wide k chunks per wave: 8 waves x 32 = 256 >= H
  constexpr int PP = 32;                  // pitch of the split-K partial tiles [8 waves][32 videos][PP]
  const int H = a.H;
  float* part = smem;
  int* sR0 = reinterpret_cast<int*>(part + 8 * 32 * PP);   // [32] first row of each video
  int* sT = sR0 + 32;                     // [32] length of each video
  int* sTg = sT + 32;                     // [1]  longest video of the group

  const int team = blockIdx.x % PK_TEAMS, slot = blockIdx.x / PK_TEAMS;
  if (slot >= a.n_active) return;
  const __amdgpu_buffer_rsrc_t lrsrc = __builtin_amdgcn_make_buffer_rsrc(a.ll, (short)0, a.ll_bytes, 0x00020000);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int u0 = slot * a.upm, nu = min(a.upm, H - u0);
  const int n_items = 2 * a.n_groups;
  int loaded_dir = -1;
  bool dead = false;   // (per wave) a wait timed out: results are invalid, state[0] and the health word say so

  float4 wreg[CPW];
  for (int item = team; item < n_items; item += PK_TEAMS) {
    const int g = item >> 1, d = item & 1;
    const int v0 = g * a.gsize, nv = min(a.gsize, a.n_seq - v0);
    __syncthreads();   // previous item fully done with LDS
    if (loaded_dir != d) {   // this lane's W_hh fragments -> registers (plain loads: weights are never written in this launch)
      if constexpr (M16) {   // column n = 16 tile + lane % 16; k = 32 wave + 8 (lane / 16) + 0..7
#pragma unroll
        for (int tile = 0; tile < 2; ++tile) {
          const int n = 16 * tile + (lane & 15);
          const float* wrow = a.whh[d] + (int64_t)(min(n & 3, 2) * H + min(u0 + (n >> 2), H - 1)) * H;
          const int k = wave * 32 + 8 * (lane >> 4);
          const bool col = (n & 3) < 3;
          wreg[2 * tile] = (col && k < H) ? *reinterpret_cast<const float4*>(wrow + k) : make_float4(0.f, 0.f, 0.f, 0.f);
          wreg[2 * tile + 1] = (col && k + 4 < H) ? *reinterpret_cast<const float4*>(wrow + k + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      } else {
        const float* wrow = a.whh[d] + (int64_t)(min(li & 3, 2) * H + min(u0 + (li >> 2), H - 1)) * H;
        const bool col = (li & 3) < 3;
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
          const int k = (wave * CPW + c) * 8 + 4 * lh;
          wreg[c] = (col && k < H) ? *reinterpret_cast<const float4*>(wrow + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      loaded_dir = d;
    }
    if (tid == 0) *sTg = 0;
    __syncthreads();
    if (tid < 32) {
      int r0 = 0, T = 0;
      if (tid < nv) { r0 = a.off[v0 + tid]; T = a.off[v0 + tid + 1] - r0; atomicMax(sTg, T); }
      sR0[tid] = r0; sT[tid] = T;
    }
    __syncthreads();
    const int Tg = *sTg;

    // epilogue role: thread (video i, unit u) for tid < 256; h_{t-1} of the unit lives in a register for the whole item
    const int ei = tid >> 3, eu = tid & 7;
    const bool erole = tid < 256 && ei < nv && eu < nu;
    const int er0 = erole ? sR0[ei] : 0, eT = erole ? sT[ei] : 0;
    const int j = u0 + eu;
    float hlast = 0.f;
    float gcur[3] = {0.f, 0.f, 0.f}, bh[3] = {0.f, 0.f, 0.f};
    if (erole && eT > 0) {
      const int64_t row = d == 0 ? er0 : er0 + eT - 1;
      const float* gp = a.G + row * (6 * H) + d * 3 * H;
#pragma unroll
      for (int q = 0; q < 3; ++q) { gcur[q] = gp[q * H + j]; bh[q] = a.bhh[d][q * H + j]; }
    }
    const int vl = M16 ? (lane & 15) : li;     // the video (row of the group) this lane feeds to the MFMAs
    const int Tl = sT[vl];

    for (int t = 0; t < Tg; ++t) {
      if (t > 0) {
        const bool need_row = t < Tl;
        const unsigned want = (unsigned)t;
        const unsigned rowb = (unsigned)((((unsigned)((t - 1) & 1) * 2u + (unsigned)d) * (unsigned)a.n_seq + (unsigned)(v0 + vl)) * (unsigned)H) * 8u;
        unsigned spins = 0;
        unsigned long long ll_t0 = 0;
        if constexpr (M16) {
          // h_{t-1}[video lane % 16][k .. k+7], k = 32 wave + 8 (lane / 16): four 16-byte loads of {value, tag} pairs, repeated until
          // every tag this lane needs says t
          const int k0 = wave * 32 + 8 * (lane >> 4);
          u32x4 va[4];
          while (true) {
            asm volatile("" ::: "memory");   // the loads below are a poll: they must be re-issued every turn
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              const unsigned o = (need_row && k0 + 2 * p < H) ? rowb + 8u * (unsigned)(k0 + 2 * p) : 0x7ffffff0u;     // beyond num_records: zeros
              va[p] = __builtin_amdgcn_raw_buffer_load_b128(lrsrc, o, 0, 16 /* sc1 */);
            }
            bool ok = true;      // branch-free tag checks (lstm_persist_kernel)
#pragma unroll
            for (int p = 0; p < 4; ++p)
              ok = ok & (((va[p][1] == want) & (va[p][3] == want)) | !(need_row && k0 + 2 * p < H));
            if (__all(ok) || dead) break;
            if (pk_ll_timed_out(spins, ll_t0)) {     // never hang the GPU: flag the failure and stop waiting
              if (lane == 0) { atomicOr(a.state, 1u); atomicOr(a.health, 1u); }
              dead = true;
            }
          }
          f32x4 hv[4];
#pragma unroll
          for (int p = 0; p < 4; ++p) hv[p] = __builtin_bit_cast(f32x4, va[p]);     // {h_k, tag, h_k+1, tag}
          f32x4 acc16[2];
#pragma unroll
          for (int tile = 0; tile < 2; ++tile) {
            acc16[tile] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float4 w0 = wreg[2 * tile], w1 = wreg[2 * tile + 1];
            acc16[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[0][0], w0.x, acc16[tile], 0, 0, 0);
            acc16[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[0][2], w0.y, acc16[tile], 0, 0, 0);
            acc16[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[1][0], w0.z, acc16[tile], 0, 0, 0);
            acc16[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[1][2], w0.w, acc16[tile], 0, 0, 0);
            acc16[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[2][0], w1.x, acc16[tile], 0, 0, 0);
            acc16[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[2][2], w1.y, acc16[tile], 0, 0, 0);
            acc16[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[3][0], w1.z, acc16[tile], 0, 0, 0);
            acc16[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[3][2], w1.w, acc16[tile], 0, 0, 0);
          }
          // C/D map of the 16x16 MFMA: row = 4 (lane / 16) + r, column = lane % 16
#pragma unroll
          for (int tile = 0; tile < 2; ++tile)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(wave * 32 + 4 * (lane >> 4) + r) * PP + 16 * tile + (lane & 15)] = acc16[tile][r];
        } else {
          // h_{t-1}[video li][k .. k+3] = two 16-byte loads of {value, tag} pairs per chunk
          u32x4 va[2 * CPW];
          while (true) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int c = 0; c < CPW; ++c) {
              const int k = (wave * CPW + c) * 8 + 4 * lh;
              const unsigned o = (need_row && k < H) ? rowb + 8u * (unsigned)k : 0x7fffffe0u;     // beyond num_records: zeros
              va[2 * c] = __builtin_amdgcn_raw_buffer_load_b128(lrsrc, o, 0, 16 /* sc1 */);
              va[2 * c + 1] = __builtin_amdgcn_raw_buffer_load_b128(lrsrc, o, 16, 16 /* sc1 */);
            }
            bool ok = true;
#pragma unroll
            for (int c = 0; c < CPW; ++c) {
              const int k = (wave * CPW + c) * 8 + 4 * lh;
              ok = ok & (((va[2 * c][1] == want) & (va[2 * c][3] == want) & (va[2 * c + 1][1] == want) & (va[2 * c + 1][3] == want)) | !(need_row && k < H));
            }
            if (__all(ok) || dead) break;
            if (pk_ll_timed_out(spins, ll_t0)) {
              if (lane == 0) { atomicOr(a.state, 1u); atomicOr(a.health, 1u); }
              dead = true;
            }
          }
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
          for (int c = 0; c < CPW; ++c) {
            const float4 bv = wreg[c];
            const f32x4 p0 = __builtin_bit_cast(f32x4, va[2 * c]), p1 = __builtin_bit_cast(f32x4, va[2 * c + 1]);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p0[0], bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p0[2], bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p1[0], bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p1[2], bv.w, acc, 0, 0, 0);
          }
          // C/D map of the 32x32 MFMA: row = (r % 4) + 8 (r / 4) + 4 (lane / 32), column = lane % 32
#pragma unroll
          for (int r = 0; r < 16; ++r) part[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * PP + li] = acc[r];
        }
        __syncthreads();
      }
      if (erole && t < eT) {
        const int64_t row = d == 0 ? er0 + t : er0 + eT - 1 - t;
        float4 ps = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t > 0) {
#pragma unroll
          for (int w8 = 0; w8 < 8; ++w8) {     // fixed order: wave 0 .. 7
            const float4 pw = *reinterpret_cast<const float4*>(&part[(w8 * 32 + ei) * PP + 4 * eu]);
            ps.x += pw.x; ps.y += pw.y; ps.z += pw.z;
          }
        }
        const float rg = fast_sigmoid(gcur[0] + (ps.x + bh[0])), zg = fast_sigmoid(gcur[1] + (ps.y + bh[1]));
        const float ghn = ps.z + bh[2];
        const float ng = fast_tanh(gcur[2] + rg * ghn);
        const float h = (1.f - zg) * ng + zg * hlast;
        const unsigned long long pkt = ((unsigned long long)(unsigned)(t + 1) << 32) | (unsigned long long)__builtin_bit_cast(unsigned, h);
        __hip_atomic_store(a.ll + ((int64_t)((t & 1) * 2 + d) * a.n_seq + (v0 + ei)) * H + j, pkt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.Hout[row * (2 * H) + d * H + j] = h;     // plain store: nobody reads the output matrix in this launch
        if (a.sv) {
          float* s = a.sv + row * (8 * H) + d * 4 * H;
          s[j] = rg; s[H + j] = zg; s[2 * H + j] = ng; s[3 * H + j] = ghn;
          a.hprev[row * (2 * H) + d * H + j] = hlast;
        }
        hlast = h;
        if (t + 1 < eT) {   // next step's input-projection slice, one step ahead
          const int64_t nrow = d == 0 ? row + 1 : row - 1;
          const float* gp = a.G + nrow * (6 * H) + d * 3 * H;
#pragma unroll
          for (int q = 0; q < 3; ++q) gcur[q] = gp[q * H + j];
        }
      }
      __syncthreads();   // the split-K partial tiles in LDS are free again (the published h needs no further signal)
    }
  }
}

// ------------------------------------------------------------------------------------------- BPTT
// Same teams and work items, steps in reverse.  Member m owns units U_m:
//   step t:  dh[i][j in U_m] = dHout[row][j] + dh(t+1) z(t+1)  (a register)  + sum over the members m' of partial_{m'}(t+1)[i][j]  (sc1 loads)
//            dn = dh (1 - z)(1 - n^2)   dz = dh (h_prev - n) z (1 - z)   dr = dn Gh_n r (1 - r)
//            dGx = [dr, dz, dn] and the n block dn r of dGh are stored for the weight-gradient GEMMs; dGh_t[i][3 gates x U_m] is the A tile in LDS
//            partial_m(t)[i][all j] = dGh_t[i][cols of U_m] . W_hh[rows of U_m][all j]   (MFMA, K = 24, one 32-column N range per wave)
//            published with sc1 stores to the exchange buffer of parity t & 1; every storing wave drains vmcnt(0), barrier, ONE lane adds to
//            the item's step counter (four shards, 128 B apart, while the items fit the state block).
// The sum over members runs in a FIXED order (deterministic).  M16 (groups of <= 16 videos): v_mfma_f32_16x16x4_f32 with the W_hh fragments
// of the wave's 32 output columns in registers (6 per tile: lane group g carries k = 6 g .. 6 g + 5 of the 24); otherwise the 32-row shape
// with the member's 24 W_hh rows in LDS.
struct GruPersistBwdArgs {
  const float* whh[2]; const float* dHout; const float* sv; const float* hprev;
  float* dgx; float* dghn; float* xchg; const int32_t* off; unsigned* state; unsigned* health;
  int32_t n_seq, H, gsize, n_groups, upm, n_active, n_items, item_words, n_shards;
};

template <bool M16>
__global__ __launch_bounds__(PK_THREADS) void gru_persist_bwd_kernel(GruPersistBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = a.H, P = H + 4;
  float* sW = smem;                       // [24][P]  W_hh rows (gate * 8 + unit) of this member, all H columns (32-row form only)
  float* sA = sW + 24 * P;                // [32][36] dGh_t of the group's videos, this member's 24 gate columns (gate * 8 + unit)
  int* sR0 = reinterpret_cast<int*>(sA + 32 * 36);
  int* sT = sR0 + 32;
  int* sTg = sT + 32;

  const int team = blockIdx.x % PK_TEAMS, slot = blockIdx.x / PK_TEAMS;
  if (slot >= a.n_active) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int u0 = slot * a.upm, nu = min(a.upm, H - u0);
  int loaded_dir = -1;
  bool dead = false;
  float wB[2][6];     // M16: this lane's W_hh fragments

  for (int item = team; item < a.n_items; item += PK_TEAMS) {
    const int g = item >> 1, d = item & 1;
    const int v0 = g * a.gsize, nv = min(a.gsize, a.n_seq - v0);
    unsigned* bar = a.state + 16 + item * a.item_words;
    __syncthreads();
    if (loaded_dir != d) {
      if constexpr (M16) {   // B fragments: W_hh[row k = 6 (lane / 16) + m of this member's 24][column 32 wave + 16 tile + lane % 16]
#pragma unroll
        for (int tile = 0; tile < 2; ++tile) {
          const int n = wave * 32 + 16 * tile + (lane & 15);
#pragma unroll
          for (int m = 0; m < 6; ++m) {
            const int r = 6 * (lane >> 4) + m;
            wB[tile][m] = n < H ? a.whh[d][(int64_t)((r >> 3) * H + min(u0 + (r & 7), H - 1)) * H + n] : 0.f;
          }
        }
      } else {
        for (int idx = tid; idx < 24 * (H >> 2); idx += PK_THREADS) {
          const int r = idx / (H >> 2), k4 = (idx % (H >> 2)) * 4;
          const int unit = min(u0 + (r & 7), H - 1);
          *reinterpret_cast<float4*>(&sW[r * P + k4]) = *reinterpret_cast<const float4*>(a.whh[d] + (int64_t)((r >> 3) * H + unit) * H + k4);
        }
      }
      loaded_dir = d;
    }
    if (tid == 0) *sTg = 0;
    __syncthreads();
    if (tid < 32) {
      int r0 = 0, T = 0;
      if (tid < nv) { r0 = a.off[v0 + tid]; T = a.off[v0 + tid + 1] - r0; atomicMax(sTg, T); }
      sR0[tid] = r0; sT[tid] = T;
    }
    __syncthreads();
    const int Tg = *sTg;

    const int ei = tid >> 3, eu = tid & 7;
    const bool erole = tid < 256 && ei < nv && eu < nu;
    const int er0 = erole ? sR0[ei] : 0, eT = erole ? sT[ei] : 0;
    const int j = u0 + eu;
    float dcarry = 0.f;     // dh(t+1) z(t+1): the direct path into h_t
    // saved activations of the step about to be processed (prefetched one step ahead)
    float sv_r = 0.f, sv_z = 0.f, sv_n = 0.f, sv_g = 0.f, sv_hp = 0.f, sv_dh = 0.f;
    float nx_r = 0.f, nx_z = 0.f, nx_n = 0.f, nx_g = 0.f, nx_hp = 0.f, nx_dh = 0.f;
    auto fetch = [&](int t) {
      const int64_t row = d == 0 ? er0 + t : er0 + eT - 1 - t;
      const float* s = a.sv + row * (8 * H) + d * 4 * H;
      nx_r = s[j]; nx_z = s[H + j]; nx_n = s[2 * H + j]; nx_g = s[3 * H + j];
      nx_hp = a.hprev[row * (2 * H) + d * H + j];
      nx_dh = a.dHout[row * (2 * H) + d * H + j];
    };
    if (erole && eT > 0 && eT - 1 == Tg - 1) {
      fetch(Tg - 1);
      sv_r = nx_r; sv_z = nx_z; sv_n = nx_n; sv_g = nx_g; sv_hp = nx_hp; sv_dh = nx_dh;
    }

    for (int t = Tg - 1; t >= 0; --t) {
      const bool have_next = erole && t - 1 >= 0 && t - 1 < eT;
      if (have_next) fetch(t - 1);
      // zero this step's A tile (rows of inactive videos and columns of absent units must contribute nothing)
      for (int idx = tid; idx < 32 * 36; idx += PK_THREADS) sA[idx] = 0.f;
      if (t < Tg - 1) {
        if (wave == 0 && !dead) {   // wait until every member published step t+1: lanes 0 .. n_shards-1 poll one shard each
          const unsigned cnt = (lane < a.n_shards && lane < a.n_active) ? (unsigned)((a.n_active - lane + a.n_shards - 1) / a.n_shards) : 0u;
          const unsigned want = (unsigned)(Tg - 1 - t) * cnt;
          unsigned spins = 0;
          while (true) {
            const unsigned v = lane < a.n_shards ? __hip_atomic_load(bar + 32 * lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
            if (__all(v >= want)) break;
            __builtin_amdgcn_s_sleep(1);
            if (++spins > PK_SPIN_LIMIT || ((spins & 1023) == 0 &&
                 __hip_atomic_load(a.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
              if (lane == 0) { atomicOr(a.state, 1u); atomicOr(a.health, 1u); }     // never hang the GPU: flag the failure and stop waiting
              dead = true; break;
            }
          }
        }
      }
      __syncthreads();
      if (erole && t < eT) {
        float dh = sv_dh + dcarry;
        if (t + 1 < eT) {   // recurrent part: fixed-order sum of the members' partials of step t+1 (sc1 loads)
          const float* xb = a.xchg + (((int64_t)((t + 1) & 1) * a.n_items + item) * 32) * 32 * H;
          const float* xp = xb + (int64_t)ei * H + j;
          const int64_t xs = (int64_t)32 * H;        // producer to producer
          float pv[32];
          if (a.n_active == 32) {     // all 32 members: no per-member predicate, 32-bit buffer offsets walked in a VGPR (lstm_persist_bwd_kernel)
            const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), (short)0, 0x7FFFFFFF, 0x00020000);
            unsigned vo = (unsigned)(xp - xb) * 4u;
            const unsigned st = (unsigned)xs * 4u;
#pragma unroll
            for (int m = 0; m < 32; ++m) { pv[m] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, vo, 0, 16 /* sc1 */)); vo += st; }
          } else {
#pragma unroll
            for (int m = 0; m < 32; ++m) pv[m] = m < a.n_active ? ld_sc1(xp + (int64_t)m * xs) : 0.f;
          }
          float rec = 0.f;
#pragma unroll
          for (int m = 0; m < 32; ++m) rec += pv[m];
          dh += rec;
        }
        const float dn = dh * (1.f - sv_z) * (1.f - sv_n * sv_n);
        const float dz = dh * (sv_hp - sv_n) * sv_z * (1.f - sv_z);
        const float dr = dn * sv_g * sv_r * (1.f - sv_r);
        const float dnr = dn * sv_r;
        dcarry = dh * sv_z;
        const int64_t row = d == 0 ? er0 + t : er0 + eT - 1 - t;
        float* dg = a.dgx + row * (6 * H) + d * 3 * H;
        dg[j] = dr; dg[H + j] = dz; dg[2 * H + j] = dn;
        a.dghn[row * (2 * H) + d * H + j] = dnr;
        sA[ei * 36 + eu] = dr; sA[ei * 36 + 8 + eu] = dz; sA[ei * 36 + 16 + eu] = dnr;
      }
      if (have_next) { sv_r = nx_r; sv_z = nx_z; sv_n = nx_n; sv_g = nx_g; sv_hp = nx_hp; sv_dh = nx_dh; }
      __syncthreads();
      if (t > 0) {   // partial_m(t) is only ever read by step t-1
        float* xo = a.xchg + ((((int64_t)(t & 1) * a.n_items + item) * 32 + slot) * 32) * H;
        if constexpr (M16) {
          // 16 videos x (this wave's 32 columns, two 16-column tiles) x K = 24: lane group g = lane / 16 carries k = 6 g .. 6 g + 5
          const int i16 = lane & 15, g4 = lane >> 4;
          float av[6];
#pragma unroll
          for (int m = 0; m < 6; ++m) av[m] = sA[i16 * 36 + 6 * g4 + m];
#pragma unroll
          for (int tile = 0; tile < 2; ++tile) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < 6; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], wB[tile][m], acc, 0, 0, 0);
            const int n = wave * 32 + 16 * tile + i16;
            if (n < H) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int i = 4 * g4 + r;      // C/D map of the 16x16 MFMA: row = 4 (lane / 16) + r, column = lane % 16
                const float pv_ = acc[r];
                if (i < nv && t < sT[i]) st_sc1(xo + (int64_t)i * H + n, pv_);
              }
            }
          }
        } else {
          const int ntile = (H + 31) >> 5;
          for (int nt = wave; nt < ntile; nt += 8) {
            const int n = nt * 32 + li, nc = min(n, H - 1);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
              const float4 av = *reinterpret_cast<const float4*>(&sA[li * 36 + kk * 8 + 4 * lh]);
              const float b0 = sW[(kk * 8 + 4 * lh + 0) * P + nc], b1 = sW[(kk * 8 + 4 * lh + 1) * P + nc];
              const float b2 = sW[(kk * 8 + 4 * lh + 2) * P + nc], b3 = sW[(kk * 8 + 4 * lh + 3) * P + nc];
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b2, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b3, acc, 0, 0, 0);
            }
            if (n < H) {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float pv_ = acc[r];
                if (i < nv && t < sT[i]) st_sc1(xo + (int64_t)i * H + n, pv_);
              }
            }
          }
        }
      }
      // publish step t: every storing wave drains its stores, then one lane signals
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) __hip_atomic_fetch_add(bar + 32 * (slot % a.n_shards), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

static int gru_check_common(int In, int H, int n_seq, const int32_t* off, int training, GruWs* L, size_t workspace_bytes, const char* who) {
  SUMK_TRY(gru_carve(In, H, n_seq, off, training, L));
  return workspace_fits(who, workspace_bytes, L->total);
}

}  // namespace sumk

using namespace sumk;

extern "C" size_t sumk_bigru_workspace_bytes(int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host, int32_t training) {
  GruWs w;
  if (gru_carve(In, H, n_seq, seq_off_host, training, &w) != SUMK_OK) return 0;
  return w.total;
}

extern "C" int sumk_bigru_layer_forward(const float* x, int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host,
                                        const int32_t* seq_off_dev, const sumk_gru_layer_weights* w, float* h_out, void* workspace,
                                        size_t workspace_bytes, int32_t training, int32_t precision, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(x && seq_off_dev && w && h_out && workspace, "bigru_forward: null pointer");
  SUMK_ARG(precision >= SUMK_PRECISION_FP32 && precision <= SUMK_PRECISION_MAX, "bigru_forward: unknown precision %d", precision);
  for (int d = 0; d < 2; ++d)
    SUMK_ARG(w->w_ih[d] && w->w_hh[d] && w->b_ih[d] && w->b_hh[d], "bigru_forward: null weight (dir %d)", d);
  GruWs L;
  SUMK_TRY(gru_check_common(In, H, n_seq, seq_off_host, training, &L, workspace_bytes, "bigru_forward"));
  SUMK_ARG(persistent_kernels_usable(), "bigru_forward: the persistent recurrence needs 256 co-resident blocks (full chip, SUMK_LSTM_PERSIST != 0); "
                                        "use the step path (sumk_gru_cell_forward)");
  unsigned* health = persist_health_word();
  SUMK_ARG(health != nullptr, "bigru_forward: cannot resolve the health word");
  char* ws = (char*)workspace;
  const int R = L.n_rows;
  float* G = (float*)(ws + L.g);
  GemmProb* prob = (GemmProb*)(ws + L.prob);

  // 1: input projection, one NT GEMM per direction into its 3H columns of G, b_ih in the epilogue
  const int small = gemm_tiles(R, 3 * H, 0) >= 512 ? 0 : 1;
  SUMK_TRY(fill_single_prob(prob, R, 3 * H, In, In, In, 6 * H, 0, small, stream));
  for (int d = 0; d < 2; ++d) {
    GemmLaunch g;
    g.A = x; g.B[0] = w->w_ih[d]; g.bias0[0] = w->b_ih[d]; g.C = G + (size_t)d * 3 * H; g.probs = prob; g.small_tile = small;
    g.total_tiles = gemm_tiles(R, 3 * H, small); g.precision = precision; g.lean = gemm_lean_ok(R, 3 * H, In, In, In);
    SUMK_TRY(launch_gemm(GEMM_NT, EPI_BIAS2, g, stream));
  }
  // 2: recurrence.  One kernel launch clears the error word and the hand-off buffer behind it (a tag of 0 matches no step).
  SUMK_TRY(persist_zero_words((unsigned*)(ws + L.pstate), (L.ll + L.ll_bytes - L.pstate) / 4, stream));
  GruPersistArgs pa;
  pa.G = G; pa.Hout = h_out;
  for (int d = 0; d < 2; ++d) { pa.whh[d] = w->w_hh[d]; pa.bhh[d] = w->b_hh[d]; }
  pa.sv = training ? (float*)(ws + L.sv) : nullptr;
  pa.hprev = training ? (float*)(ws + L.hprev) : nullptr;
  pa.off = seq_off_dev; pa.state = (unsigned*)(ws + L.pstate); pa.health = health;
  pa.n_seq = n_seq; pa.H = H; pa.gsize = L.gsize; pa.n_groups = L.n_groups;
  pa.upm = std::min(8, (H + 31) / 32); pa.n_active = (H + pa.upm - 1) / pa.upm;
  pa.ll = (unsigned long long*)(ws + L.ll); pa.ll_bytes = (int32_t)L.ll_bytes;
  const bool m16 = L.gsize <= 16;
  prof_begin(SUMK_PROF_LSTM_REC, stream);
  // 33 KB used; > 80 KB keeps one block per CU
  SUMK_TRY(m16 ? persist_launch<gru_persist_kernel<true>>(&pa, 96 * 1024, stream) : persist_launch<gru_persist_kernel<false>>(&pa, 96 * 1024, stream));
  prof_end(SUMK_PROF_LSTM_REC, stream);
  return SUMK_OK;
}

extern "C" int sumk_bigru_layer_backward(const float* x, const float* h_out, const float* dh_out, int32_t In, int32_t H, int32_t n_seq,
                                         const int32_t* seq_off_host, const int32_t* seq_off_dev, const sumk_gru_layer_weights* w,
                                         const sumk_gru_layer_grads* gr, float* dx, void* workspace, size_t workspace_bytes,
                                         int32_t precision, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(precision >= SUMK_PRECISION_FP32 && precision <= SUMK_PRECISION_MAX, "bigru_backward: unknown precision %d", precision);
  SUMK_ARG(x && h_out && dh_out && seq_off_dev && w && gr && workspace, "bigru_backward: null pointer");
  for (int d = 0; d < 2; ++d)
    SUMK_ARG(w->w_ih[d] && w->w_hh[d] && gr->w_ih[d] && gr->w_hh[d] && gr->b_ih[d] && gr->b_hh[d], "bigru_backward: null weight/grad (dir %d)", d);
  GruWs L;
  SUMK_TRY(gru_check_common(In, H, n_seq, seq_off_host, 1, &L, workspace_bytes, "bigru_backward (needs the training-mode forward's workspace)"));
  SUMK_ARG(persistent_kernels_usable(), "bigru_backward: the persistent recurrence needs 256 co-resident blocks");
  unsigned* health = persist_health_word();
  SUMK_ARG(health != nullptr, "bigru_backward: cannot resolve the health word");
  char* ws = (char*)workspace;
  const int R = L.n_rows;
  float* dgx = (float*)(ws + L.dgx);
  float* dghn = (float*)(ws + L.dghn);
  float* hprev = (float*)(ws + L.hprev);
  float* slab = (float*)(ws + L.slab);
  float* colpart = (float*)(ws + L.colpart);
  GemmProb* prob = (GemmProb*)(ws + L.prob);
  GemmProb* psk = (GemmProb*)(ws + L.prob_sk);

  SUMK_TRY(persist_zero_words((unsigned*)(ws + L.pstate_b), PSTATE_WORDS, stream));
  {
    GruPersistBwdArgs pa;
    pa.whh[0] = w->w_hh[0]; pa.whh[1] = w->w_hh[1]; pa.dHout = dh_out; pa.sv = (const float*)(ws + L.sv); pa.hprev = hprev;
    pa.dgx = dgx; pa.dghn = dghn; pa.xchg = (float*)(ws + L.xchg);
    pa.off = seq_off_dev; pa.state = (unsigned*)(ws + L.pstate_b); pa.health = health;
    pa.n_seq = n_seq; pa.H = H; pa.gsize = L.gsize; pa.n_groups = L.n_groups; pa.n_items = 2 * L.n_groups;
    pa.upm = std::min(8, (H + 31) / 32); pa.n_active = (H + pa.upm - 1) / pa.upm;
    const bool shard = pk_items_shard(pa.n_items);
    pa.item_words = shard ? PSTATE_ITEM_WORDS : 1; pa.n_shards = shard ? 4 : 1;
    const bool m16 = L.gsize <= 16;
    // 24 x 260 + 32 x 36 floats + tables = 30 KB used; > 80 KB keeps one block per CU
    SUMK_TRY(m16 ? persist_launch<gru_persist_bwd_kernel<true>>(&pa, 96 * 1024, stream) : persist_launch<gru_persist_bwd_kernel<false>>(&pa, 96 * 1024, stream));
  }
  // weight gradients: dW_ih[d] += dGx_d^T X (both directions in one split-K launch); dW_hh[d] += dGh_d^T h_prev_d with
  // dGh_d = [dr | dz] of dGx_d (rows 0 .. 2H of W_hh) and the stored n block (rows 2H .. 3H)
  {
    float* out[4] = {gr->w_ih[0], gr->w_ih[1], nullptr, nullptr};
    SUMK_TRY(gemm_tn_splitk_accum(dgx, 6 * H, x, In, 6 * H, In, R, slab, L.slab_elems, psk, 64, out, 3 * H, In, 1.f, stream, precision));
  }
  for (int d = 0; d < 2; ++d) {
    float* out_rz[4] = {gr->w_hh[d], nullptr, nullptr, nullptr};
    SUMK_TRY(gemm_tn_splitk_accum(dgx + (size_t)d * 3 * H, 6 * H, hprev + (size_t)d * H, 2 * H, 2 * H, H, R, slab, L.slab_elems, psk, 64,
                                  out_rz, 2 * H, H, 1.f, stream, precision));
    float* out_n[4] = {gr->w_hh[d] + (size_t)2 * H * H, nullptr, nullptr, nullptr};
    SUMK_TRY(gemm_tn_splitk_accum(dghn + (size_t)d * H, 2 * H, hprev + (size_t)d * H, 2 * H, H, H, R, slab, L.slab_elems, psk, 64,
                                  out_n, H, H, 1.f, stream, precision));
  }
  {   // b_ih: column sums of dGx; b_hh: those of its r and z blocks, and of the stored n block of dGh
    const ReduceSeg segs[4] = {{0, 3 * H, gr->b_ih[0]}, {0, 2 * H, gr->b_hh[0]}, {3 * H, 3 * H, gr->b_ih[1]}, {3 * H, 2 * H, gr->b_hh[1]}};
    SUMK_TRY(colsum_multi(dgx, 6 * H, R, 6 * H, colpart, 128, segs, 4, stream));
    const ReduceSeg segn[2] = {{0, H, gr->b_hh[0] + 2 * H}, {H, H, gr->b_hh[1] + 2 * H}};
    SUMK_TRY(colsum_multi(dghn, 2 * H, R, 2 * H, colpart, 128, segn, 2, stream));
  }
  if (dx) {  // dX = dGx_fwd W_ih_fwd + dGx_rev W_ih_rev
    const int small = gemm_tiles(R, In, 0) >= 512 ? 0 : 1;
    SUMK_TRY(fill_single_prob(prob + 1, R, In, 3 * H, 6 * H, In, In, 0, small, stream));
    for (int d = 0; d < 2; ++d) {
      GemmLaunch g;
      g.A = dgx + (size_t)d * 3 * H; g.B[0] = w->w_ih[d]; g.C = dx; g.probs = prob + 1; g.small_tile = small;
      g.total_tiles = gemm_tiles(R, In, small); g.precision = precision;
      SUMK_TRY(launch_gemm(GEMM_NN, d == 0 ? EPI_NONE : EPI_ACCUM, g, stream));
    }
  }
  return SUMK_OK;
}

// Synchronous health check of the persistent GRU kernels that last ran on this workspace (sumk_bilstm_check's twin).
extern "C" int sumk_bigru_check(const void* workspace, int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host,
                                int32_t training, int32_t after_backward, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SUMK_ARG(workspace, "bigru_check: null workspace");
  GruWs L;
  SUMK_TRY(gru_carve(In, H, n_seq, seq_off_host, training, &L));
  unsigned flags[2] = {0u, 0u};
  SUMK_HIP(hipMemcpyAsync(&flags[0], (const char*)workspace + L.pstate, 4, hipMemcpyDeviceToHost, stream));
  if (training && after_backward) SUMK_HIP(hipMemcpyAsync(&flags[1], (const char*)workspace + L.pstate_b, 4, hipMemcpyDeviceToHost, stream));
  SUMK_HIP(hipStreamSynchronize(stream));
  if (flags[0] != 0u || flags[1] != 0u) {
    set_error("bigru: persistent recurrence kernel timed out waiting for a team member (forward flag %u, backward flag %u); "
              "outputs are invalid", flags[0], flags[1]);
    return SUMK_ERR_HIP;
  }
  return SUMK_OK;
}
