// ce_lww.h -- LWWReg<u64, u64> (crdts 7: struct LWWReg<V, M> { val: V, marker: M }, Op = LWWReg,
// apply(op) = merge(op) = update(val, marker): taken when self.marker < marker, so an equal marker
// keeps the incumbent): the op grammar shared by host and device, the per-file records and the
// launch interface of ce_lww.hip, driven by ce_lww_host.cpp.
//
// The fold is an argmax, not a max: of the gated files' ops the winner is the one with the largest
// marker, and among equals the first in apply order (read_remote_ops keeps the batch's order,
// lib.rs:512-541): the lowest file index, then the lowest index in its file.  Every decode path
// leaves one record (marker, val) per file at rec[f], the file's own winner -- (0, 0) when the
// file is gated out, fails, or holds no op with a non-zero marker (such an op can never replace
// anything: the default register's marker is 0) -- and k_lww_reduce picks the batch's by (marker
// descending, file index ascending).  Nothing is folded atomically, so no schedule of the waves
// can change the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_common.h"
#include "ce_kernels.h"

namespace ce {

// One op.  LWWReg { val, marker } (derive(Deserialize)): a map keyed "val" / "marker" (or by field
// index) in any order, unknown keys ignored, a repeated or a missing field rejected; or an array of
// exactly 2.  Both fields: any non-negative integer form (rd_u64).  Returns as parse_dot: 1 ok,
// 0 decode error, -1 nesting too deep for the bounded skip.
template <typename R>
CE_HD int parse_lww_op(R& r, uint64_t* val, uint64_t* marker) {
  static constexpr const char* kF[2] = {"val", "marker"};
  if (r.i >= r.n) return 0;
  const uint8_t m = rb(r, r.i);
  uint64_t cnt;
  const bool arr = is_array_marker(m);  // the fields in order, no keys
  if (arr) {
    if (!rd_array_hdr(r, &cnt) || cnt != 2) return 0;
  } else if (!rd_map_hdr(r, &cnt)) {
    return 0;
  }
  unsigned seen = 0;
  for (uint64_t k = 0; k < cnt; k++) {
    int f = arr ? (int)k : rd_field<2>(r, kF);
    if (f < 0) return 0;
    if (f == 2) {
      int s = rd_skip(r);
      if (s <= 0) return s;
      continue;
    }
    if (seen & (1u << f)) return 0;
    seen |= 1u << f;
    if (!rd_u64(r, f == 0 ? val : marker)) return 0;
  }
  return seen == 3u ? 1 : 0;
}

// encoded length of a u64 in its smallest form: 1, 2, 3, 5 or 9
CE_HD uint32_t lww_uint_width(uint8_t m) {
  return m <= 0x7f ? 1u : (m >= 0xcc && m <= 0xcf) ? 1u + (1u << (m - 0xcc)) : 0u;
}

struct LwwRec {  // a file's winner (16 bytes)
  unsigned long long marker, val;
};

// what the fused open's LWW grammar (ce_fused.hip k_open_fold_v3<false, true, false, false, true>)
// reads through DecodeArgs.lw (device memory): the record column and the launch's file counts,
// paths[0] uniform, [1] general (shared with k_decode_lww), [2] files decoded in the open,
// [3] files decoded by k_decode_lww
struct LwwFused {
  LwwRec* rec;      // [n], zeroed before the launch; a file writes its own row only
  uint32_t* paths;
};

struct LwwDecodeArgs {
  const uint8_t* pt;          // plaintext blob (FileParams.out_off / len)
  const FileParams* params;
  int32_t* status;
  uint32_t n;
  const uint8_t* supported;   // n_supported * 16 bytes
  uint32_t n_supported;
  const uint8_t* apply;       // 1 = this file's ops count (version gate)
  const uint8_t* only;        // null, or per file: decode only files with only[i] != 0
  int large_only;             // only files of more than one page (the fused open took the others)
  LwwRec* rec;
  uint32_t* paths;
};

// one wave per file: data version, array header, the uniform-stride or the general path; statuses
// CE_ERR_PT_LEN / CE_ERR_PT_VERSION / CE_ERR_DECODE into a.status, the file's winner into a.rec
hipError_t launch_decode_lww(hipStream_t s, const LwwDecodeArgs& a, uint32_t grid_waves);

// k_lww_reduce: the argmax of rec[0..n) by (marker descending, file index ascending).  Blocks of
// kLwwBlock threads take tiles of kLwwTile records grid-stride (tile t to block t mod grid) and
// leave one partial each; the final stage, one block, reduces the partials into out[0].  The grid
// is min(tiles, kLwwMaxBlocks), or grid_cap (the test-only CE_TEST_GRID_CAP) when that is smaller.
static constexpr uint32_t kLwwBlock = 256;
static constexpr uint32_t kLwwTile = 256;
static constexpr uint32_t kLwwMaxBlocks = 64;
struct LwwPartial {
  unsigned long long marker, val;
  uint32_t idx, pad;
};
// part: kLwwMaxBlocks partials of scratch; out: one record.  n >= 1
hipError_t launch_lww_reduce(hipStream_t s, const LwwRec* rec, uint32_t n, LwwPartial* part, LwwRec* out,
                             uint32_t grid_cap);

// k_lww_reduce_keyed: the sharded ingest's reduce (ce_core_lwwreg_ingest_ops_device_sharded).  A
// rank holds a share of the batch, and the whole batch's apply order is (index in the shared
// writer list, version): record i is read together with its address (fa[i], fv[i]) and the argmax
// is by (marker descending, fa ascending, fv ascending, local index ascending) -- the keys
// themselves, since a share's writer runs may come in any order; the local index only separates
// two files given the same address, which Storage cannot produce.  The winner leaves with its
// address, so the best of the ranks' winners under the same order is the whole batch's.  Same
// tiling, grid and grid_cap as k_lww_reduce; marker 0 never wins: out = kLwwKeyedNone then.
struct LwwKeyed {  // a share's winner (32 bytes): what the ranks exchange
  unsigned long long marker, val, fa, fv;
};
static constexpr LwwKeyed kLwwKeyedNone = {0ull, 0ull, ~0ull, ~0ull};
struct LwwKeyedPartial {
  unsigned long long marker, val, fv;
  uint32_t fa, idx;
};
// a beats b in the batch's apply order among equal markers, and by marker first
CE_HD bool lww_keyed_better(unsigned long long ma, unsigned long long faa, unsigned long long fva, uint32_t ia,
                            unsigned long long mb, unsigned long long fab, unsigned long long fvb, uint32_t ib) {
  if (ma != mb) return ma > mb;
  if (faa != fab) return faa < fab;
  if (fva != fvb) return fva < fvb;
  return ia < ib;
}
// part: kLwwMaxBlocks partials of scratch; out: one record.  n >= 1
hipError_t launch_lww_reduce_keyed(hipStream_t s, const LwwRec* rec, const uint32_t* fa, const uint64_t* fv,
                                   uint32_t n, LwwKeyedPartial* part, LwwKeyed* out, uint32_t grid_cap);

}  // namespace ce
