// ce_gset_device.h -- the GSet hash set's device side (ce_gset.h): probe and insert, shared by
// ce_gset.hip's kernels and the fused open's GSet grammar (ce_fused.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_gset.h"

namespace ce {

__device__ __forceinline__ unsigned long long ld_slot(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_word(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t gs_hash(unsigned long long k) {
  k *= 0x9E3779B97F4A7C15ull;
  return (uint32_t)(k >> 32) ^ (uint32_t)k;
}

// key != 0.  The table is at most half full, so the probe ends.
__device__ __forceinline__ bool gs_contains(const GsTable& t, unsigned long long key) {
  for (uint32_t i = gs_hash(key) & t.mask;; i = (i + 1) & t.mask) {
    const unsigned long long v = ld_slot(&t.slots[i]);
    if (v == key) return true;
    if (v == 0) return false;
  }
}

__device__ __forceinline__ void gs_insert(const GsTable& t, unsigned long long key) {
  if (key == 0) {  // the empty pattern's own member: out of band
    if (ld_word(&t.meta[kGsZero]) == 0) atomicExch(&t.meta[kGsZero], 1u);
    return;
  }
  for (uint32_t i = gs_hash(key) & t.mask;; i = (i + 1) & t.mask) {
    const unsigned long long v = ld_slot(&t.slots[i]);
    if (v == key) return;
    if (v != 0) continue;
    // an empty slot: reserve a unit of the count, then claim.  The count (reservations included)
    // never passes the limit, so claimed slots never do.
    if (ld_word(&t.meta[kGsOverflow])) return;
    if (atomicAdd(&t.meta[kGsCount], 1u) >= t.limit) {
      atomicSub(&t.meta[kGsCount], 1u);
      atomicExch(&t.meta[kGsOverflow], 1u);
      return;
    }
    const unsigned long long prev = atomicCAS(&t.slots[i], 0ull, key);
    if (prev == 0) return;
    atomicSub(&t.meta[kGsCount], 1u);  // another lane took the slot
    if (prev == key) return;
  }
}

// a decoded member of a gated file: known members are found read-only in the committed table,
// absent ones are claimed in the batch table
__device__ __forceinline__ void gs_put(const GsTable& committed, const GsTable& batch, unsigned long long v) {
  if (v != 0 && gs_contains(committed, v)) return;
  if (v == 0 && ld_word(&committed.meta[kGsZero])) return;
  gs_insert(batch, v);
}

}  // namespace ce
