// ce_gset_write.hip -- the GSet op-file writer (gfx950): a member column in HBM laid out as many
// small op files, and the CE_GSET_APPLY_NEW_ONLY filter over the sorted column (ce_gset.h).
//
// File i's clear text is VersionBytes(data_version, to_vec_named(Vec<u64>)) (crdt-enc/src/lib.rs:
// 670-671): 16 bytes of data version, a fixarray or array16 header, the members big-endian in their
// smallest unsigned form.  With at most kGsFileMembers members it is at most one 4096-byte page,
// the size the readers' fused open decodes in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_gset.h"
#include "ce_gset_device.h"
#include "ce_opfile_device.h"

namespace ce {
namespace {

constexpr uint32_t kGroup = kOpFileGroup;
constexpr uint32_t kWaveFiles = 4;    // files per wave and trip
constexpr uint32_t kPage = 4096;      // the longest clear text: 16 + 3 + 9 * kGsFileMembers
static_assert(16 + 3 + 9 * kGsFileMembers <= kPage, "a file's clear text is one page");
// the wave's files lie back to back in the clear blob; they are staged at the same offset mod 16
constexpr uint32_t kStageBytes = kWaveFiles * kPage + 16;

// members of file f (0 past the last file)
__device__ __forceinline__ uint32_t file_count(const GsFilesArgs& a, uint32_t f) {
  if (f >= a.L.n_files) return 0;
  const unsigned long long left = a.n - (unsigned long long)f * a.per_file;
  return left < a.per_file ? (uint32_t)left : a.per_file;
}

// The size pass: one 16-lane group per file sums its members' widths.  Every lane of a block runs
// the same trips, so the shuffles see whole groups.
__global__ __launch_bounds__(256) void k_gs_file_sizes(GsFilesArgs a) {
  const uint32_t sub = threadIdx.x & (kGroup - 1);
  const uint32_t per_block = 256 / kGroup;
  const uint32_t F = a.L.n_files;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.L.clen[F] = a.L.xlen[F] = 0;
  for (uint32_t base = blockIdx.x * per_block; base < F; base += gridDim.x * per_block) {
    const uint32_t f = base + threadIdx.x / kGroup;
    const uint32_t cnt = file_count(a, f);
    const uint32_t sum = group_width_sum(a.members + (unsigned long long)f * a.per_file, cnt, sub);
    if (f < F && sub == 0) opfile_set_sizes(a.L, f, 16 + arr_hdr_len(cnt) + sum);
  }
}

// The encoder: one wave per block, kWaveFiles files per trip.  Group q stages file f0 + q in LDS:
// the data version, the header, then its members (group_put_members).  The wave's files are one
// byte range [c0, c1) of the clear blob, staged at c0's offset mod 16 (opfile_flush).
__global__ __launch_bounds__(64) void k_gs_files_encode(GsFilesArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
  const uint32_t lane = threadIdx.x, q = lane / kGroup, sub = lane & (kGroup - 1);
  const uint32_t F = a.L.n_files;
  const uint32_t trips = (F + kWaveFiles - 1) / kWaveFiles;
  const uint32_t rounds = (a.per_file + kGroup - 1) / kGroup;
  for (uint32_t w = blockIdx.x; w < trips; w += gridDim.x) {
    const uint32_t f0 = w * kWaveFiles;
    const uint32_t f1 = f0 + kWaveFiles < F ? f0 + kWaveFiles : F;
    const uint32_t c0 = a.L.coff[f0], c1 = a.L.coff[f1];  // c1 - c0 <= kWaveFiles * kPage
    const uint32_t f = f0 + q;
    const uint32_t cnt = file_count(a, f);
    uint32_t at = 0;  // the file's first byte in the stage
    if (f < F) {
      at = (c0 & 15) + (a.L.coff[f] - c0);
      if (sub == 0) {
        opfile_publish_offsets(a.L, f);
        const uint32_t hc = arr_hdr_len(cnt);
        for (uint32_t k = 0; k < hc; k++) stage[at + 16 + k] = arr_hdr_byte(cnt, hc, k);
      }
      stage[at + sub] = a.L.dv[sub];
    }
    group_put_members(stage, at + 16 + arr_hdr_len(cnt), a.members + (unsigned long long)f * a.per_file, cnt, rounds, sub);
    __syncthreads();
    opfile_flush(stage, a.L.clear, c0 & ~15u, c0, c1, lane);
    __syncthreads();  // the stage is rewritten by the next trip
  }
}

// first probes of kNewProbes elements issued together (k_gs_contains' form); a collision walks on
constexpr int kNewProbes = 4;

__global__ __launch_bounds__(256) void k_gs_new_mark(GsTable t, const unsigned long long* s, uint32_t n,
                                                     uint32_t* keep) {
  const uint32_t zero = ld_word(&t.meta[kGsZero]);
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  if (blockIdx.x == 0 && threadIdx.x == 0) keep[n] = 0;
  for (unsigned long long base = (unsigned long long)blockIdx.x * 256 + threadIdx.x; base < n;
       base += kNewProbes * stride) {
    unsigned long long v[kNewProbes], slot[kNewProbes];
    bool first[kNewProbes];
#pragma unroll
    for (int j = 0; j < kNewProbes; j++) {
      const unsigned long long i = base + (unsigned long long)j * stride;
      v[j] = i < n ? s[i] : 0ull;
      first[j] = i < n && (i == 0 || s[i - 1] != v[j]);
    }
    // (a lane past the end probes the slot of key 0: inside the table, never looked at)
#pragma unroll
    for (int j = 0; j < kNewProbes; j++) slot[j] = ld_slot(&t.slots[gs_hash(v[j]) & t.mask]);
#pragma unroll
    for (int j = 0; j < kNewProbes; j++) {
      const unsigned long long i = base + (unsigned long long)j * stride;
      if (i >= n) continue;
      bool held = false;
      if (first[j]) {
        if (v[j] == 0) held = zero != 0;  // the member 0 is held out of band
        else if (slot[j] == v[j]) held = true;
        else if (slot[j] != 0) held = gs_contains(t, v[j]);
      }
      keep[i] = first[j] && !held ? 1u : 0u;
    }
  }
}

__global__ __launch_bounds__(256) void k_gs_new_compact(const unsigned long long* s, const uint32_t* keep,
                                                        const uint32_t* pos, uint32_t n, unsigned long long* out) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    if (keep[i]) out[pos[i]] = s[i];
}

}  // namespace

hipError_t launch_gs_file_sizes(hipStream_t s, const GsFilesArgs& a) {
  if (a.L.n_files == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gs_file_sizes, dim3(grid_blocks(a.L.n_files, 256 / kGroup, 4096)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gs_files_encode(hipStream_t s, const GsFilesArgs& a, uint32_t grid_cap) {
  if (a.L.n_files == 0) return hipSuccess;
  // 16 KiB of LDS a block: nine blocks a CU
  hipLaunchKernelGGL(k_gs_files_encode, dim3(grid_blocks(a.L.n_files, kWaveFiles, grid_cap ? grid_cap : 256 * 9)), dim3(64),
                     0, s, a);
  return hipGetLastError();
}

hipError_t launch_gs_new_mark(hipStream_t s, GsTable t, const unsigned long long* sorted, uint32_t n, uint32_t* keep) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gs_new_mark, dim3(grid_blocks(n, 256 * kNewProbes, 2048)), dim3(256), 0, s, t, sorted, n, keep);
  return hipGetLastError();
}

hipError_t launch_gs_new_compact(hipStream_t s, const unsigned long long* sorted, const uint32_t* keep,
                                 const uint32_t* pos, uint32_t n, unsigned long long* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gs_new_compact, dim3(grid_blocks(n, 256, 4096)), dim3(256), 0, s, sorted, keep, pos, n, out);
  return hipGetLastError();
}

}  // namespace ce
