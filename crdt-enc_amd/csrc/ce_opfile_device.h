// ce_opfile_device.h -- the op-file writers' shared device pieces (ce_opfile.h): a file's two
// sizes, its two published offsets, the staged flush, and the 16-lane group's member loops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_opfile.h"

namespace ce {

constexpr uint32_t kOpFileGroup = 16;  // lanes per file, the readers' geometry

// file f's clear length, and what its envelope's two bin headers add at that length
__device__ __forceinline__ void opfile_set_sizes(const OpFileLayout& L, uint32_t f, uint32_t len) {
  L.clen[f] = len;
  L.xlen[f] = (uint32_t)(16 + sealed_len(len) - len - kOpFileSealBase);
}

// the seal's two offsets of file f; the last file's lane also writes the closing pair
__device__ __forceinline__ void opfile_publish_offsets(const OpFileLayout& L, uint32_t f) {
  const uint32_t F = L.n_files, cf = L.coff[f];
  L.offs[f] = cf;
  L.file_offs[f] = (unsigned long long)cf + (unsigned long long)f * kOpFileSealBase + L.xoff[f];
  if (f == F - 1) {
    L.offs[F] = L.coff[F];
    L.file_offs[F] = (unsigned long long)L.coff[F] + (unsigned long long)F * kOpFileSealBase + L.xoff[F];
  }
}

// One wave's staged bytes into the clear blob.  stage[b] belongs at clear[w0 + b], w0 a multiple
// of 16; the bytes at clear offsets [lo, hi) leave (w0 <= lo, hi within the stage), whole chunks
// as aligned 16-byte stores, the first and last partial chunk -- shared with the neighbouring
// waves' ranges -- byte by byte.  Between two __syncthreads of the caller.
__device__ __forceinline__ void opfile_flush(const uint8_t* stage, uint8_t* clear, uint32_t w0, uint32_t lo, uint32_t hi,
                                             uint32_t lane) {
  uint8_t* g16 = clear + w0;
  for (uint32_t c = lane * 16; w0 + c < hi; c += 64 * 16) {
    const uint32_t g = w0 + c;
    if (g >= lo && g + 16 <= hi) {
      *reinterpret_cast<uint4*>(g16 + c) = *reinterpret_cast<const uint4*>(stage + c);
    } else {
      const uint32_t c0 = g < lo ? lo - w0 : c, c1 = g + 16 < hi ? c + 16 : hi - w0;
      for (uint32_t b = c0; b < c1; b++) g16[b] = stage[b];
    }
  }
}

// The 16-lane group's loops over members m[0, cnt), lane sub taking members sub + 16 j.  Every
// lane of the group runs the same trips, so the shuffles see whole groups.
// the sum of the members' widths, in every lane
__device__ __forceinline__ uint32_t group_width_sum(const unsigned long long* m, uint32_t cnt, uint32_t sub) {
  uint32_t sum = 0;
  for (uint32_t e = sub; e < cnt; e += kOpFileGroup) sum += uint_width(m[e]);
#pragma unroll
  for (int d = 1; d < (int)kOpFileGroup; d <<= 1) sum += (uint32_t)__shfl_xor((int)sum, d, kOpFileGroup);
  return sum;
}
// the members written from stage[run] on, 16 to a round (rounds >= ceil(cnt / 16), the same in
// every lane), a prefix of the widths carrying the running byte offset, which is returned
__device__ __forceinline__ uint32_t group_put_members(uint8_t* stage, uint32_t run, const unsigned long long* m,
                                                      uint32_t cnt, uint32_t rounds, uint32_t sub) {
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t e = r * kOpFileGroup + sub;
    const bool has = e < cnt;
    const unsigned long long x = has ? m[e] : 0ull;
    const uint32_t wd = has ? uint_width(x) : 0u;
    uint32_t incl = wd;
#pragma unroll
    for (int d = 1; d < (int)kOpFileGroup; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, d, kOpFileGroup);
      if (sub >= (uint32_t)d) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, kOpFileGroup - 1, kOpFileGroup);
    if (has) put_uint(stage + run + incl - wd, x);
    run += total;
  }
  return run;
}

}  // namespace ce
