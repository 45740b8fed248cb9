// ce_orswot_write.hip -- the Orswot add-op writer (gfx950): a member column in HBM laid out as
// files of Add ops by the local actor, and the fold's add columns of the same ops
// (ce_orswot_write.h).
//
// File i's clear text is VersionBytes(data_version, to_vec_named(Vec<orswot::Op<u64, Uuid>>))
// (crdt-enc/src/lib.rs:670-671).  The host admits only shapes whose worst case is one 4096-byte
// page, so a file is staged whole in LDS.
//
// The work unit follows the op's length, in the size pass and in the encoder alike: ops of fewer
// than kOwGroupOps members (a fixarray of members; C3's one-member ops among them) take a lane
// each, which needs no cross-lane step at all -- the op's start comes from the scanned lengths;
// longer ops (add_all's shape) take a 16-lane group each (group_width_sum, group_put_members), as
// the GSet writer lays out a file.  The file size pass is the shared one (ce_opfile.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_opfile_device.h"
#include "ce_orswot_write.h"

namespace ce {
namespace {

constexpr uint32_t kGroup = kOpFileGroup;
constexpr uint32_t kWaveFiles = 4;  // files per wave and trip
// the wave's files lie back to back in the clear blob; they are staged at the same offset mod 16
constexpr uint32_t kStageBytes = kWaveFiles * kOwPage + 16;

// ops of file f, members of op j (0 past the last)
__device__ __forceinline__ uint32_t file_ops(const OwArgs& a, uint32_t f) {
  if (f >= a.L.n_files) return 0;
  const unsigned long long left = a.n_ops - (unsigned long long)f * a.opf;
  return left < a.opf ? (uint32_t)left : a.opf;
}
__device__ __forceinline__ uint32_t op_count(const OwArgs& a, unsigned long long j) {
  if (j >= a.n_ops) return 0;
  const unsigned long long left = a.n - j * a.per_op;
  return left < a.per_op ? (uint32_t)left : a.per_op;
}

// The op size pass.  Short ops: a lane per op.  Long ops: a 16-lane group per op sums its members'
// widths; every lane of a block runs the same trips, so the shuffles see whole groups.
__global__ __launch_bounds__(256) void k_ow_op_sizes(OwArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) a.olen[a.n_ops] = 0;
  if (a.per_op < kOwGroupOps) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x; j < a.n_ops; j += stride) {
      const uint32_t cnt = op_count(a, j);
      const unsigned long long* m = a.members + j * a.per_op;
      uint32_t sum = 0;
      for (uint32_t e = 0; e < cnt; e++) sum += uint_width(m[e]);
      a.olen[j] = kOwFixedBytes + uint_width(a.c0 + 1 + j) + arr_hdr_len(cnt) + sum;
    }
    return;
  }
  const uint32_t sub = threadIdx.x & (kGroup - 1);
  const uint32_t per_block = 256 / kGroup;
  const unsigned long long stride = (unsigned long long)gridDim.x * per_block;
  for (unsigned long long base = (unsigned long long)blockIdx.x * per_block; base < a.n_ops; base += stride) {
    const unsigned long long j = base + threadIdx.x / kGroup;
    const uint32_t cnt = op_count(a, j);
    const uint32_t sum = group_width_sum(a.members + j * a.per_op, cnt, sub);
    if (j < a.n_ops && sub == 0) a.olen[j] = kOwFixedBytes + uint_width(a.c0 + 1 + j) + arr_hdr_len(cnt) + sum;
  }
}

// A short op whole, by one lane: the constant head, the counter, a7 "members", the fixarray
// header and the members.
__device__ __forceinline__ void write_op_lane(uint8_t* p, const OwArgs& a, const uint8_t* head, unsigned long long j) {
#pragma unroll
  for (uint32_t k = 0; k < kOwHeadBytes; k++) p[k] = head[k];
  p += kOwHeadBytes;
  p += put_uint(p, a.c0 + 1 + j);
#pragma unroll
  for (uint32_t k = kOwHeadBytes; k < kOwFixedBytes; k++) p[k - kOwHeadBytes] = head[k];
  p += kOwFixedBytes - kOwHeadBytes;
  const uint32_t cnt = op_count(a, j);  // (< kOwGroupOps: a fixarray)
  *p++ = (uint8_t)(0x90 | cnt);
  const unsigned long long* m = a.members + j * a.per_op;
  for (uint32_t e = 0; e < cnt; e++) p += put_uint(p, m[e]);
}

// The encoder: one wave per block, kWaveFiles files per trip, group q staging file f0 + q in LDS.
// Short ops: lane sub writes ops sub, sub + 16, ... of its file, each at the start the scanned
// lengths give it.  Long ops: the group writes its file's ops one after another -- the up to 63
// bytes before the members spread over the lanes, then the members (group_put_members); every
// lane of the wave runs opf x rounds trips.  The wave's files are one byte range [b0, b1) of the
// clear blob, staged at b0's offset mod 16 (opfile_flush).
__global__ __launch_bounds__(64) void k_ow_encode(OwArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
  const uint8_t* head = reinterpret_cast<const uint8_t*>(a.head);
  const uint32_t lane = threadIdx.x, q = lane / kGroup, sub = lane & (kGroup - 1);
  const uint32_t F = a.L.n_files;
  const uint32_t trips = (F + kWaveFiles - 1) / kWaveFiles;
  const bool lane_ops = a.per_op < kOwGroupOps;
  const uint32_t op_rounds = (a.opf + kGroup - 1) / kGroup;
  const uint32_t mem_rounds = (a.per_op + kGroup - 1) / kGroup;
  for (uint32_t w = blockIdx.x; w < trips; w += gridDim.x) {
    const uint32_t f0 = w * kWaveFiles;
    const uint32_t f1 = f0 + kWaveFiles < F ? f0 + kWaveFiles : F;
    const uint32_t b0 = a.L.coff[f0], b1 = a.L.coff[f1];  // b1 - b0 <= kWaveFiles * kOwPage
    const uint32_t f = f0 + q;
    const uint32_t nops = file_ops(a, f);
    const unsigned long long j0 = (unsigned long long)f * a.opf;
    uint32_t body = 0, ob0 = 0;  // the first op's byte in the stage, and in the scanned lengths
    if (f < F) {
      const uint32_t at = (b0 & 15) + (a.L.coff[f] - b0);
      if (sub == 0) {
        opfile_publish_offsets(a.L, f);
        const uint32_t hv = arr_hdr_len(nops);
        for (uint32_t k = 0; k < hv; k++) stage[at + 16 + k] = arr_hdr_byte(nops, hv, k);
      }
      stage[at + sub] = a.L.dv[sub];
      body = at + 16 + arr_hdr_len(nops);
      ob0 = a.ooff[j0];
    }
    if (lane_ops) {
      for (uint32_t r = 0; r < op_rounds; r++) {
        const uint32_t k = r * kGroup + sub;
        if (k < nops) write_op_lane(stage + body + (a.ooff[j0 + k] - ob0), a, head, j0 + k);
      }
    } else {
      for (uint32_t k = 0; k < a.opf; k++) {  // (the same trips in every lane: whole groups shuffle)
        const bool has_op = k < nops;
        const unsigned long long j = j0 + k;
        const uint32_t cnt = has_op ? op_count(a, j) : 0u;
        uint32_t run = 0;
        if (has_op) {
          const uint32_t at = body + (a.ooff[j] - ob0);
          const unsigned long long ctr = a.c0 + 1 + j;
          const uint32_t wc = uint_width(ctr), hc = arr_hdr_len(cnt);
          const uint32_t pre = kOwFixedBytes + wc + hc;  // <= 63
          for (uint32_t b = sub; b < pre; b += kGroup) {
            uint8_t v;
            if (b < kOwHeadBytes) v = head[b];
            else if (b < kOwHeadBytes + wc) v = uint_byte(ctr, wc, b - kOwHeadBytes);
            else if (b < kOwFixedBytes + wc) v = head[b - wc];
            else v = arr_hdr_byte(cnt, hc, b - kOwFixedBytes - wc);
            stage[at + b] = v;
          }
          run = at + pre;
        }
        group_put_members(stage, run, a.members + j * a.per_op, cnt, mem_rounds, sub);
      }
    }
    __syncthreads();
    opfile_flush(stage, a.L.clear, b0 & ~15u, b0, b1, lane);
    __syncthreads();  // the stage is rewritten by the next trip
  }
}

__global__ __launch_bounds__(256) void k_ow_cols(OwCols a) {
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.add_mbeg[a.n_add] = (uint32_t)a.n;
    a.rm_cbeg[0] = a.rm_mbeg[0] = 0;
  }
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {
    a.add_mem[i] = a.members[i];
    if (i < a.n_add) {  // add i: members from i * span, inside op i * span / per_op
      const unsigned long long first = i * a.span;
      a.add_actor[i] = a.actor_id;
      a.add_ctr[i] = a.c0 + 1 + first / a.per_op;
      a.add_mbeg[i] = (uint32_t)first;
      a.applied[i] = 1;
      a.excl[i] = i ? a.c0 + 1 + (first - a.span) / a.per_op : 0ull;
    }
  }
}

}  // namespace

hipError_t launch_ow_op_sizes(hipStream_t s, const OwArgs& a) {
  if (a.n_ops == 0) return hipSuccess;
  const uint32_t per_block = a.per_op < kOwGroupOps ? 256u : 256u / kGroup;
  hipLaunchKernelGGL(k_ow_op_sizes, dim3(grid_blocks(a.n_ops, per_block, 4096)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ow_encode(hipStream_t s, const OwArgs& a, uint32_t grid_cap) {
  if (a.L.n_files == 0) return hipSuccess;
  // one wave and 16,400 bytes of LDS a block: nine blocks resident a CU (160 KiB), the LDS the
  // limit -- nine waves of staging and byte stores a CU, no other resource near its bound
  hipLaunchKernelGGL(k_ow_encode, dim3(grid_blocks(a.L.n_files, kWaveFiles, grid_cap ? grid_cap : 256 * 9)), dim3(64), 0,
                     s, a);
  return hipGetLastError();
}

hipError_t launch_ow_cols(hipStream_t s, const OwCols& a) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ow_cols, dim3(grid_blocks(a.n, 256, 4096)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace ce
