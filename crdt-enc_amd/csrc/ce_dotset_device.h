// ce_dotset_device.h -- the dot-set member table's device side (ce_dotset.h): the hash and the
// lookup, shared by ce_dotset.hip's kernels and the Rm-op writer's mark pass (ce_orswot_rm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_dotset.h"

namespace ce {

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

__device__ __forceinline__ unsigned long long ld_volatile(const unsigned long long* p) {
  return __atomic_load_n(p, __ATOMIC_RELAXED);
}

// member handle (index into mkey) or kDsEmpty when absent (insert = false).  A member lives in
// the primary table (smask + 1 slots, sized for the members actually present: small enough to stay
// in L2) unless the kMemberWindow slots of its probe sequence there were all taken by other members
// when it was inserted; then it lives in the overflow table (as large as the pair table, so it
// never fills).  Slots never empty again, so a lookup that meets an empty slot in the window knows
// the member is in neither table, and every thread inserting one member takes the same branch.
constexpr uint32_t kMemberWindow = 32;

__device__ __forceinline__ unsigned long long member_reserved(const DsTables& t) {
  return (unsigned long long)t.smask + 1 + t.mmask + 1;
}

__device__ unsigned long long member_find(const DsTables& t, unsigned long long m, bool insert) {
  if (m == kDsEmpty) return member_reserved(t);  // reserved bucket
  const unsigned long long x = mix64(m);
  uint32_t h = (uint32_t)x & t.smask;
  for (uint32_t probe = 0; probe < kMemberWindow; probe++) {
    const unsigned long long k = ld_volatile(t.mkey + h);
    if (k == m) return h;
    if (k == kDsEmpty) {
      if (!insert) return kDsEmpty;
      const unsigned long long prev = atomicCAS(t.mkey + h, kDsEmpty, m);
      if (prev == kDsEmpty || prev == m) return h;
    }
    h = (h + 1) & t.smask;
  }
  const unsigned long long base = (unsigned long long)t.smask + 1;
  unsigned long long* ov = t.mkey + base;
  h = (uint32_t)(x >> 32) & t.mmask;
  for (uint32_t probe = 0; probe <= t.mmask; probe++) {
    const unsigned long long k = ld_volatile(ov + h);
    if (k == m) return base + h;
    if (k == kDsEmpty) {
      if (!insert) return kDsEmpty;
      const unsigned long long prev = atomicCAS(ov + h, kDsEmpty, m);
      if (prev == kDsEmpty || prev == m) return base + h;
    }
    h = (h + 1) & t.mmask;
  }
  atomicAdd(t.live + 2, 1u);  // table full (host sizes it to <= 50% load)
  return kDsEmpty;
}

}  // namespace ce
