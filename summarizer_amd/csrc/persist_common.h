// Shared by the persistent recurrence kernels (lstm.hip, gru_persist.hip): vector types, the gate math of the per-step latency chain,
// the bounded-wait constants of the hand-off protocol (written out at the top of the "persistent recurrence" section of lstm.hip) and
// the host-side helpers that lstm.hip owns.
#pragma once
#include "sumk_internal.h"

namespace sumk {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Gate math of the persistent H <= 256 recurrence, whose per-step latency chain contains it: v_exp_f32 / v_rcp_f32 forms (a few ulp:
// ~3e-7 relative for the sigmoid, ~1e-7 ABSOLUTE for tanh) instead of the library expf / IEEE division / tanhf (~170 instructions per
// step and thread against ~30).  tanh(x) = 1 - 2 / (1 + e^{2x}) saturates correctly at both ends (e^{2x} -> inf gives 1, -> 0 gives -1).
// (round 6: __frcp_rn is the CORRECTLY ROUNDED reciprocal -- hipcc expands it to the v_div_scale / v_div_fmas / v_div_fixup sequence, 5 x ~10
//  instructions in every cell update; __builtin_amdgcn_rcpf is the bare v_rcp_f32 these forms were written for: 1 ulp)
__device__ __forceinline__ float fast_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
__device__ __forceinline__ float fast_tanh(float v) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * v)); }

constexpr int PK_THREADS = 512;
constexpr int PK_TEAMS = 8;
constexpr unsigned PK_SPIN_LIMIT = 1u << 20;   // ~1 s of polling; after one timeout the block stops waiting altogether
// The flag-in-data hand-offs poll with their OWN data loads (a turn = four to thirty-two sc1 loads, ~1 us), so a turn count is a poor
// clock: they share the counter protocol's ~1 s budget in WALL time -- s_memrealtime, the 100 MHz constant counter -- read every 256
// turns, the first time at turn 256 (a healthy wait ends long before).  (A count of PK_SPIN_LIMIT / 16 turns was tens of ms: resume skew after a CWSR preemption, or several ranks time-slicing
// one GPU, could have tripped it on a healthy run.)
constexpr unsigned long long PK_WAIT_TICKS = 100000000ull;
__device__ __forceinline__ bool pk_ll_timed_out(unsigned& spins, unsigned long long& t0) {     // (the clock is first read at turn 256: nothing on the fast path)
  if ((++spins & 255u) != 0u) return false;
  const unsigned long long now = __builtin_amdgcn_s_memrealtime();
  if (spins == 256u) { t0 = now; return false; }
  return now - t0 > PK_WAIT_TICKS;
}

__device__ __forceinline__ float ld_sc1(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// lstm.hip: 256 co-resident blocks are available (full chip, SUMK_LSTM_PERSIST != 0); the device address of g_sumk_health (nullptr if
// the symbol cannot be resolved); zero_words_kernel over `words` 32-bit words
bool persistent_kernels_usable();
unsigned* persist_health_word();
int persist_zero_words(unsigned* p, size_t words, hipStream_t stream);

}  // namespace sumk
