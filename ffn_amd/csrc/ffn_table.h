// Open-addressing hash table over u64 keys, shared by ffn_labels.hip (joint-id
// histograms, relabelling), ffn_partitions.hip (label sizes), ffn_decision.hip
// (per-pair minimum), ffn_analysis.hip (per-point id counts) and
// ffn_metrics.hip (contingency and skeleton tables).  Not part of the C-ABI.
//
// A table is `mask + 1` (a power of two) u64 key slots, all kEmptyKey when
// empty; the payload arrays are the caller's, indexed by the slot returned.
// Two levels: a kernel may collect its keys in a table of its block in LDS
// first (block_claim) and flush that into the global one (table_insert) at its
// end; a key that finds the block's table crowded goes to the global one at
// once.  The host sizes the global table by trying (table_grow).
#ifndef FFN_TABLE_H_
#define FFN_TABLE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ffn_unit.h"

namespace ffn_table {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u64 kEmptyKey = ~0ull;
constexpr u32 kBackground = 0xffffffffu;
constexpr u32 kMaxProbes = 1u << 14;  // global table: give up -> grow + retry
constexpr int kLdsProbes = 16;        // block table: give up -> global table

__device__ __forceinline__ u32 mix64(u64 k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return (u32)k;
}

// Slot of `key` in the global table, inserting it if absent.
__device__ __forceinline__ u32 table_insert(u64* keys, u32 mask, u64 key,
                                            int* overflow) {
  u32 slot = mix64(key) & mask;
  for (u32 probe = 0; probe < kMaxProbes; ++probe) {
    u64 prev = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
    if (prev == kEmptyKey) prev = atomicCAS(&keys[slot], kEmptyKey, key);
    if (prev == kEmptyKey || prev == key) return slot;
    slot = (slot + 1) & mask;
    // table already known to be too small: stop probing, the host regrows it
    if ((probe & 255) == 255 &&
        __hip_atomic_load(overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return kBackground;
  }
  *overflow = 1;
  return kBackground;
}

// Slot of `key` in a block's LDS table of kSlots keys, claiming a free one if
// absent; -1 after kLdsProbes probes (crowded).  The payload arrays and the
// atomic on them are the caller's.
template <int kSlots>
__device__ __forceinline__ int block_claim(u64* skeys, u64 key) {
  u32 s = mix64(key) & (kSlots - 1);
  // kept a loop: unrolled 16 times at every call site it is several times the
  // code, and contact_min_kernel, which claims for 7 candidates, ran 1.7 % slower
#pragma unroll 1
  for (int probe = 0; probe < kLdsProbes; ++probe) {
    const u64 prev = atomicCAS(&skeys[s], kEmptyKey, key);
    if (prev == kEmptyKey || prev == key) return (int)s;
    s = (s + 1) & (kSlots - 1);
  }
  return -1;
}

// Slot of `key` (read only); kBackground if absent.
__device__ __forceinline__ u32 table_find(const u64* keys, u32 mask, u64 key) {
  u32 slot = mix64(key) & mask;
  for (u32 probe = 0; probe < kMaxProbes; ++probe) {
    const u64 k = keys[slot];
    if (k == key) return slot;
    if (k == kEmptyKey) return kBackground;
    slot = (slot + 1) & mask;
  }
  return kBackground;
}

// Lanes holding the same key as their left neighbour form a run; only the
// first lane of a run (the leader) touches a hash table.  Returns the leader
// mask; `valid` lanes must form a prefix of the wave.
__device__ __forceinline__ u64 run_leaders(u64 key, bool valid, int lane) {
  const u64 left = __shfl_up(key, 1);
  return __ballot(valid && (lane == 0 || left != key));
}

// Lanes of the run that starts at leader `lane`: up to the next leader or the
// end of the wave (intersect with the ballot of what is to be counted).
__device__ __forceinline__ u64 run_mask(u64 leaders, int lane) {
  const u64 above = lane == 63 ? 0ull : leaders & (~0ull << (lane + 1));
  const u64 below_end = above ? ((1ull << __builtin_ctzll(above)) - 1) : ~0ull;
  return below_end & (~0ull << lane);
}

// The occupied slots as dense arrays, in no particular order; *n_out counts
// all of them, only the first `cap` are written.  out_slot may be NULL.  (A
// template, so that only the units that launch it carry it.)
template <typename Count>
__global__ void table_compact_kernel(const u64* keys, const Count* counts,
                                     u32 nslots, u64* out_key, Count* out_count,
                                     u32* out_slot, u32 cap, u32* n_out) {
  const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  const u64 k = keys[s];
  if (k == kEmptyKey) return;
  const u32 j = atomicAdd(n_out, 1u);
  if (j < cap) {
    out_key[j] = k;
    out_count[j] = counts[s];
    if (out_slot) out_slot[j] = s;
  }
}

// Host: fills `tables` global tables of *nslots slots each (one array) through
// `launch(mask)` until none overflows.  A round clears the keys and the two
// flag words at `flags`; `launch` prepares its payload, queues its kernels on
// `stream` and times them.  Word 0 is table_insert's: 1 after the round means
// too small, and *nslots (kept by the caller from call to call) grows fourfold
// unless it has reached `limit`.  Any other flag state ends the loop as well;
// it comes back in `state` for the caller to judge (a table is complete only
// if both words are 0).
template <typename Launch>
int table_grow(hipStream_t stream, ffn_unit::DevBuf& keys, size_t tables,
               u32* nslots, u32 limit, int* flags, int state[2],
               Launch launch) {
  for (;;) {
    const size_t bytes = tables * *nslots * sizeof(u64);
    U_OK(ffn_unit::ensure(keys, bytes));
    U_TRY(hipMemsetAsync(keys.p, 0xff, bytes, stream));
    U_TRY(hipMemsetAsync(flags, 0, 2 * sizeof(int), stream));
    U_OK(launch(*nslots - 1));
    U_TRY(hipMemcpyAsync(state, flags, 2 * sizeof(int), hipMemcpyDeviceToHost,
                         stream));
    U_TRY(hipStreamSynchronize(stream));
    if (state[0] != 1 || state[1]) return FFN_OK;
    if (*nslots >= limit)
      return ffn_set_error(FFN_ERR_ARG, "id table overflow at %u slots",
                           *nslots);
    *nslots <<= 2;
  }
}

}  // namespace ffn_table

#endif  // FFN_TABLE_H_
