// Device-side open-addressing hash table over u64 keys, shared by the label
// kernels (ffn_labels.hip: joint-id histograms, relabelling) and the decision
// point kernels (ffn_decision.hip: per-pair minimum).  Not part of the C-ABI.
//
// A table is `mask + 1` (a power of two) u64 key slots, all kEmptyKey when
// empty; the payload arrays are the caller's, indexed by the slot returned.
#ifndef FFN_TABLE_H_
#define FFN_TABLE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ffn_table {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u64 kEmptyKey = ~0ull;
constexpr u32 kBackground = 0xffffffffu;
constexpr u32 kMaxProbes = 1u << 14;  // global table: give up -> grow + retry

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

}  // namespace ffn_table

#endif  // FFN_TABLE_H_
