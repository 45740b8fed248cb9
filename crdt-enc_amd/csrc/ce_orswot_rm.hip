// ce_orswot_rm.hip -- the Orswot Rm-op writer (gfx950): a member column in HBM laid out as files
// of Rm ops, each carrying its member's entry clock as read from the committed tables, and the
// fold's removal columns of the same ops (ce_orswot_rm.h).
//
// The clocks come from two scans of the pair table.  The first counts, per representative, the
// live pairs and their encoded bytes, which is all the size passes need; the second writes every
// such pair as (representative << rank_bits | UUID rank, counter), and one radix sort over those
// keys puts each op's entries together and in the wire's order.  A lane takes an op in the size
// pass and in the encoder: the sums a longer op would need a group for were made by the scan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_dotset_device.h"
#include "ce_opfile_device.h"
#include "ce_orswot_rm.h"

namespace ce {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kWin = 16384;  // the encoder's staging window: bytes of LDS a wave

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// first[handle] = the lowest position that names the handle's member (a vector atomic min on a
// word a member slot); members 0 and ~0 take the lookup's own paths
__global__ void __launch_bounds__(kBlock) k_rm_mark(RmArgs a) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    const unsigned long long h = member_find(a.t, a.members[i], false);
    a.hnd[i] = h == kDsEmpty ? kRmNoHandle : (uint32_t)h;
    if (h != kDsEmpty) atomicMin(a.first + h, i);
  }
}

__global__ void __launch_bounds__(kBlock) k_rm_unmark(RmArgs a) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    const uint32_t h = a.hnd[i];
    if (h != kRmNoHandle) a.first[h] = 0xffffffffu;
  }
}

// one scan of the pair table: a live pair of a marked handle is counted for its representative
__global__ void __launch_bounds__(kBlock) k_rm_count(RmArgs a) {
  const uint32_t slots = a.t.pmask + 1;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < slots; i += gridDim.x * kBlock) {
    const unsigned long long key = a.t.pkey[i];
    if (key == kDsEmpty) continue;
    const unsigned long long v = a.t.cur[i];
    if (v == 0) continue;
    const uint32_t r = a.first[key >> kDsActorBits];
    if (r >= a.n) continue;
    atomicAdd(a.cnt + r, 1u);
    atomicAdd(a.ebytes + r, 18u + uint_width(v));
  }
}

// every position's representative and whether it is written, and the call's totals (every lane of
// a wave runs the same trips: the sums see whole waves)
__global__ void __launch_bounds__(kBlock) k_rm_keep(RmArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) a.keep[a.n] = 0;
  unsigned long long ents = 0, op_ents = 0, ops = 0;
  for (uint32_t i0 = blockIdx.x * kBlock; i0 < a.n; i0 += gridDim.x * kBlock) {
    const uint32_t i = i0 + threadIdx.x;
    if (i >= a.n) continue;
    const uint32_t h = a.hnd[i];
    uint32_t r = h == kRmNoHandle ? i : a.first[h];
    if (r > i) r = i;  // (never: the mark pass saw position i)
    const uint32_t k = a.cnt[r];
    const uint32_t kp = a.live_only ? (r == i && k > 0 ? 1u : 0u) : 1u;
    a.rep[i] = r;
    a.keep[i] = kp;
    ents += a.cnt[i];
    op_ents += kp ? k : 0u;
    ops += kp;
  }
  ents = wave_sum64(ents);
  op_ents = wave_sum64(op_ents);
  ops = wave_sum64(ops);
  if ((threadIdx.x & 63) == 0) {
    if (ents) atomicAdd(a.tot + kRmTotEntries, ents);
    if (op_ents) atomicAdd(a.tot + kRmTotOpEntries, op_ents);
    if (ops) atomicAdd(a.tot + kRmTotOps, ops);
  }
}

__global__ void __launch_bounds__(kBlock) k_rm_scatter(RmArgs a) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    const uint32_t j = a.kpos[i];
    if (a.keep[i] && j < a.n_ops) a.op_pos[j] = i;
  }
}

// the second scan: the counted pairs written out, in no order, under the keys the sort orders
__global__ void __launch_bounds__(kBlock) k_rm_gather(RmArgs a) {
  const uint32_t slots = a.t.pmask + 1;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < slots; i += gridDim.x * kBlock) {
    const unsigned long long key = a.t.pkey[i];
    if (key == kDsEmpty) continue;
    const unsigned long long v = a.t.cur[i];
    if (v == 0) continue;
    const uint32_t r = a.first[key >> kDsActorBits];
    if (r >= a.n) continue;
    const unsigned long long at = atomicAdd(a.tot + kRmTotGather, 1ull);
    if (at >= a.n_ent) continue;
    const uint32_t aid = (uint32_t)(key & ((1u << kDsActorBits) - 1));
    const uint32_t rank = aid < a.n_ids ? a.rank_of_id[aid] : 0u;
    a.key[at] = ((unsigned long long)r << a.rank_bits) | rank;
    a.idx[at] = (uint32_t)at;
    a.ctr[at] = v;
  }
}

// the sorted entries as (actor id, counter) columns: the encoder's and the fold's
__global__ void __launch_bounds__(kBlock) k_rm_entries(RmArgs a) {
  const unsigned long long mask = (1ull << a.rank_bits) - 1;
  for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < a.n_ent; e += gridDim.x * kBlock) {
    const uint32_t rank = (uint32_t)(a.skey[e] & mask), at = a.sidx[e];
    a.s_actor[e] = rank < a.n_ids ? a.id_of_rank[rank] : 0u;
    a.s_ctr[e] = at < a.n_ent ? a.ctr[at] : 0ull;
  }
}

// ops of file f (0 past the last)
__device__ __forceinline__ uint32_t file_ops(const RmArgs& a, uint32_t f) {
  if (f >= a.L.n_files) return 0;
  const uint32_t left = a.n_ops - f * a.opf;
  return left < a.opf ? left : a.opf;
}

// The op size pass, a lane per op: the scan left its entries' count and bytes.
__global__ void __launch_bounds__(kBlock) k_rm_op_sizes(RmArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) a.olen[a.n_ops] = 0;
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.n_ops; j += gridDim.x * kBlock) {
    const uint32_t p = a.op_pos[j], r = a.rep[p];
    a.olen[j] = kRmFixedBytes + rm_map_hdr(a.cnt[r]) + a.ebytes[r] + uint_width(a.members[p]);
  }
}

// a lane's view of the staging window: bytes at clear offsets [lo, hi) land in stage, the rest of
// what the lane walks over is dropped
struct RmOut {
  uint8_t* stage;
  uint32_t w0, lo, span, pos;
  __device__ __forceinline__ void put(uint8_t b) {
    if (pos - lo < span) stage[pos - w0] = b;
    pos++;
  }
};

// The encoder: one wave a block, kRmRunOps consecutive ops a trip, a lane an op.  The run's bytes
// are one range [b0, b1) of the clear blob -- a file's data version and Vec header belong to the
// lane of the file's first op -- staged in LDS a window of kWin bytes at a time, at the same
// offset mod 16 as in the blob (opfile_flush).  A lane walks its op once per window the op
// touches, stepping over the entries before the window by their widths.
__global__ void __launch_bounds__(64) k_rm_encode(RmArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWin];
  const uint8_t* head = reinterpret_cast<const uint8_t*>(a.head);
  const uint32_t lane = threadIdx.x;
  const uint32_t runs = (a.n_ops + kRmRunOps - 1) / kRmRunOps;
  for (uint32_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const uint32_t j0 = run * kRmRunOps;
    const uint32_t cnt_run = a.n_ops - j0 < kRmRunOps ? a.n_ops - j0 : kRmRunOps;
    const uint32_t j = j0 + lane;
    const bool mine = lane < cnt_run;
    uint32_t wstart = 0, wend = 0, at = 0, nops_f = 0, k = 0, e0 = 0, wm = 0;
    unsigned long long m = 0;
    bool file_head = false;
    if (mine) {
      const uint32_t f = j / a.opf, kf = j - f * a.opf;
      nops_f = file_ops(a, f);
      const uint32_t cf = a.L.coff[f];
      at = cf + 16 + arr_hdr_len(nops_f) + (a.ooff[j] - a.ooff[f * a.opf]);
      wend = at + (a.ooff[j + 1] - a.ooff[j]);
      file_head = kf == 0;
      wstart = file_head ? cf : at;
      if (file_head) opfile_publish_offsets(a.L, f);
      const uint32_t p = a.op_pos[j], r = a.rep[p];
      k = a.cnt[r];
      e0 = a.ebeg[r];
      if (e0 > a.n_ent || k > a.n_ent - e0) k = 0;  // (never: the scans agree)
      m = a.members[p];
      wm = uint_width(m);
    }
    const uint32_t b0 = (uint32_t)__shfl((int)wstart, 0);
    const uint32_t b1 = (uint32_t)__shfl((int)wend, (int)cnt_run - 1);
    for (uint32_t w0 = b0 & ~15u; w0 < b1; w0 += kWin) {
      const uint32_t lo = b0 > w0 ? b0 : w0, hi = b1 < w0 + kWin ? b1 : w0 + kWin;
      if (mine && wstart < hi && wend > lo) {
        RmOut o{stage, w0, lo, hi - lo, wstart};
        if (file_head) {
#pragma unroll
          for (uint32_t b = 0; b < 16; b++) o.put(a.L.dv[b]);
          const uint32_t hv = arr_hdr_len(nops_f);
          for (uint32_t b = 0; b < hv; b++) o.put(arr_hdr_byte(nops_f, hv, b));
        }
#pragma unroll
        for (uint32_t b = 0; b < kRmHeadBytes; b++) o.put(head[b]);
        if (k <= 15) {
          o.put((uint8_t)(0x80 | k));
        } else if (k <= 65535) {
          o.put(0xde);
          o.put((uint8_t)(k >> 8));
          o.put((uint8_t)k);
        } else {
          o.put(0xdf);
          o.put((uint8_t)(k >> 24));
          o.put((uint8_t)(k >> 16));
          o.put((uint8_t)(k >> 8));
          o.put((uint8_t)k);
        }
        for (uint32_t e = e0; e < e0 + k; e++) {
          if (o.pos >= hi) break;
          const unsigned long long c = a.s_ctr[e];
          const uint32_t wd = uint_width(c);
          if (o.pos + 18 + wd <= lo) {  // wholly before the window
            o.pos += 18 + wd;
            continue;
          }
          const uint32_t id = a.s_actor[e];
          const uint4 u = *reinterpret_cast<const uint4*>(a.uuid_of_id + 16ull * (id < a.n_ids ? id : 0u));
          const uint32_t uw[4] = {u.x, u.y, u.z, u.w};
          o.put(0xc4);
          o.put(0x10);
#pragma unroll
          for (uint32_t b = 0; b < 16; b++) o.put((uint8_t)(uw[b >> 2] >> (8 * (b & 3))));
          for (uint32_t b = 0; b < wd; b++) o.put(uint_byte(c, wd, b));
        }
        o.pos = wend - wm - (kRmFixedBytes - kRmHeadBytes);  // a7 "members" 91 <member>
#pragma unroll
        for (uint32_t b = kRmHeadBytes; b < kRmFixedBytes; b++) o.put(head[b]);
        for (uint32_t b = 0; b < wm; b++) o.put(uint_byte(m, wm, b));
      }
      __syncthreads();
      opfile_flush(stage, a.L.clear, w0, lo, hi, lane);
      __syncthreads();  // the stage is rewritten by the next window
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_rm_cols(RmCols a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.add_mbeg[0] = 0;
    a.rm_cbeg[a.n] = a.n_ent;
    a.rm_mbeg[a.n] = a.n;
  }
  const uint32_t top = a.n > a.n_ent ? a.n : a.n_ent;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < top; i += gridDim.x * kBlock) {
    if (i < a.n) {
      a.rm_cbeg[i] = a.ebeg[i];
      a.rm_mbeg[i] = i;
      a.rm_mem[i] = a.members[i];
    }
    if (i < a.n_ent) {
      a.rmc_actor[i] = a.s_actor[i];
      a.rmc_ctr[i] = a.s_ctr[i];
    }
  }
}

}  // namespace

hipError_t launch_rm_mark(hipStream_t s, const RmArgs& a) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_mark, dim3(grid_blocks(a.n, kBlock, 4096)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_unmark(hipStream_t s, const RmArgs& a) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_unmark, dim3(grid_blocks(a.n, kBlock, 4096)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_count(hipStream_t s, const RmArgs& a) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_count, dim3(grid_blocks((uint64_t)a.t.pmask + 1, kBlock, 2048)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_keep(hipStream_t s, const RmArgs& a) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_keep, dim3(grid_blocks(a.n, kBlock, 1024)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_scatter(hipStream_t s, const RmArgs& a) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_scatter, dim3(grid_blocks(a.n, kBlock, 4096)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_gather(hipStream_t s, const RmArgs& a) {
  if (a.n_ent == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_gather, dim3(grid_blocks((uint64_t)a.t.pmask + 1, kBlock, 2048)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_entries(hipStream_t s, const RmArgs& a) {
  if (a.n_ent == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_entries, dim3(grid_blocks(a.n_ent, kBlock, 4096)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_op_sizes(hipStream_t s, const RmArgs& a) {
  if (a.n_ops == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_op_sizes, dim3(grid_blocks(a.n_ops, kBlock, 4096)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_encode(hipStream_t s, const RmArgs& a, uint32_t grid_cap) {
  if (a.n_ops == 0) return hipSuccess;
  // one wave and 16 KiB of LDS a block: nine blocks resident a CU (160 KiB), the LDS the limit
  hipLaunchKernelGGL(k_rm_encode, dim3(grid_blocks(a.n_ops, kRmRunOps, grid_cap ? grid_cap : 256 * 9)), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rm_cols(hipStream_t s, const RmCols& a) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_cols, dim3(grid_blocks(a.n > a.n_ent ? a.n : a.n_ent, kBlock, 4096)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace ce
