// Shared by the persistent recurrence kernels (lstm.hip, gru_persist.hip): vector types, the gate math of the per-step latency chain,
// the bounded-wait constants of the hand-off protocol (written out at the top of the "persistent recurrence" section of lstm.hip), the
// host-side helpers that lstm.hip owns, and the host arithmetic the layers' workspace plans share (state block, group size, sequence
// scan, workspace check, cooperative launch).
#pragma once
#include "sumk_internal.h"
#include <algorithm>

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

// ------------------------------------------------------------------------------------------- host: what the layers' plans share
// State block of a persistent launch.  Word 0: the per-call error flag; words 16..: step counters per work item -- one word each, or
// (lstm_wide2_kernel always, the BPTTs while the items fit) four shards on lines of their own, 128 words per item.  The last
// PSTATE_SPARE_WORDS words are unused: the sharded layouts stay clear of them (their eligibility bounds, and so which kernel a batch
// gets, are as measured).
constexpr int PSTATE_WORDS = 16 + 16384;
constexpr int PSTATE_SPARE_WORDS = 512;
constexpr int PSTATE_ITEM_WORDS = 128;        // a sharded item
inline bool pk_items_fit(int n_items) { return n_items <= PSTATE_WORDS - 16; }
inline bool pk_items_shard(int n_items) { return n_items * PSTATE_ITEM_WORDS <= PSTATE_WORDS - 16 - PSTATE_SPARE_WORDS; }

// videos per work item of the H <= 256 recurrences: a batch spreads over the 8 teams in both directions, and at most 32 fit the LDS map
// (gsize x (H + 4) floats in front of the partial tiles)
inline int pk_group_size(int n_seq) { return std::min(32, std::max(1, (2 * n_seq + PK_TEAMS - 1) / PK_TEAMS)); }

// Packed batch on the host: seq_off[0] = 0 and every sequence has a step.  `who` prefixes the messages; `item` / `steps` name a sequence
// and its steps in the caller's words ("video" / "frames").
inline int scan_sequences(int n_seq, const int32_t* off, const char* who, const char* item, const char* steps, int32_t* n_rows, int32_t* t_max) {
  SUMK_ARG(n_seq > 0 && off != nullptr && off[0] == 0, "%s: empty batch / seq_off[0] != 0", who);
  int tmax = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int T = off[s + 1] - off[s];
    SUMK_ARG(T > 0, "%s: %s %d has %d %s", who, item, s, T, steps);
    tmax = T > tmax ? T : tmax;
  }
  *n_rows = off[n_seq]; *t_max = tmax;
  return SUMK_OK;
}

// `note` follows the two sizes (" (needs the training-mode forward's workspace)")
inline int workspace_fits(const char* who, size_t have, size_t need, const char* note = "") {
  if (have >= need) return SUMK_OK;
  set_error("%s: workspace %zu < required %zu%s", who, have, need, note);
  return SUMK_ERR_WORKSPACE;
}

// Cooperative launch of one persistent kernel instance over the chip: 256 blocks of PK_THREADS, `shmem` bytes of dynamic LDS (callers ask
// for > 80 KB to keep one block per CU).  The instance's dynamic-LDS ceiling is raised the first time it is launched on a device.
template <auto Kernel>
int persist_launch(void* args, size_t shmem, hipStream_t stream) {
  SUMK_TRY(lds_opt_in<Kernel>(160 * 1024));
  void* kargs[] = {args};
  SUMK_HIP(hipLaunchCooperativeKernel((const void*)Kernel, dim3(PK_TEAMS * 32), dim3(PK_THREADS), kargs, (unsigned)shmem, stream));
  return SUMK_OK;
}

}  // namespace sumk
