// ce_orswot_rm.h -- the Orswot Rm-op writer's launch interface (ce_orswot_rm.hip), driven by
// ds_rm_members_device (ce_dotset_host.cpp).
//
// A member column in HBM becomes one Rm op a member, the reference's Orswot::rm(member, ctx) with
// ctx = contains(member).derive_rm_ctx(): Rm { clock: entries[member], members: [member] }, every
// clock read from the committed state before anything changes.  The ops are cut, in order, into
// files of ops_per_file ops (the last may hold fewer); file i's clear text is
//   data version (16) || Vec header || its ops, each
//   81 a2 "Rm" 82 a5 "clock" 81 a4 "dots" <map header of k> k x (c4 10 <actor> <counter>)
//   a7 "members" 91 <member>
// with every integer in its smallest unsigned form and the entries ascending by UUID bytes:
// 26 + hm(k) + sum (18 + w(counter)) + w(member) bytes an op.  An op's length depends on the
// state, so a file has no fixed bound and may pass a page.
//
// Position i of the column is represented by the lowest position that names the same member
// (itself when the member is absent): the representative's entries are the clock of every
// position it stands for.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_common.h"
#include "ce_dotset.h"
#include "ce_opfile.h"

namespace ce {

static constexpr uint32_t kRmHeadBytes = 17;   // an op up to its clock's map header
static constexpr uint32_t kRmFixedBytes = 26;  // ... and a7 "members" 91 behind the entries
static constexpr uint32_t kRmNoHandle = 0xffffffffu;
static constexpr uint32_t kRmRunOps = 64;      // ops a wave encodes per trip, a lane each

// the most clear text n_ops ops over e_ops entries (counted once an op) in F files can take
CE_HD constexpr uint64_t rm_clear_bound(uint64_t n_ops, uint64_t e_ops, uint64_t F) {
  return F * (16 + 3) + n_ops * (kRmFixedBytes + 5 + 9) + e_ops * (18 + 9);
}

// totals the host reads (u64 words)
enum { kRmTotEntries = 0, kRmTotOpEntries = 1, kRmTotOps = 2, kRmTotGather = 3, kRmTotN = 4 };

struct RmArgs {
  DsTables t;
  const unsigned long long* members;  // [n] the column
  uint32_t n;
  uint32_t live_only;           // CE_ORSWOT_RM_LIVE_ONLY
  uint32_t* first;              // a word per member slot, all ones outside a call: the lowest
                                // position that names the slot's member
  uint32_t* hnd;                // [n] member handle of position i (kRmNoHandle: absent)
  uint32_t* cnt;                // [n + 1] live pairs of representative i (0 elsewhere, and at n)
  uint32_t* ebytes;             // [n] their encoded bytes, 18 + w(counter) each
  uint32_t* rep;                // [n] representative of position i
  uint32_t* keep;               // [n + 1] 1 where position i is written as an op, keep[n] = 0
  const uint32_t* kpos;         // [n + 1] exclusive sums of keep
  const uint32_t* ebeg;         // [n + 1] exclusive sums of cnt: representative i's sorted entries
  uint32_t* op_pos;             // [n_ops] the position op j writes
  unsigned long long* tot;      // [kRmTotN], zeroed beforehand
  // the gather and the sort
  const uint32_t* rank_of_id;   // UUID-order rank of each stable actor id
  const uint32_t* id_of_rank;
  const uint8_t* uuid_of_id;    // 16 bytes an id
  int rank_bits;
  uint32_t n_ids;               // ids the three tables cover
  uint32_t n_ent;               // live pairs of the representatives (tot[kRmTotEntries])
  unsigned long long* key;      // [n_ent] representative << rank_bits | rank, in scan order
  uint32_t* idx;                // [n_ent] 0, 1, ... (the sort's value column)
  unsigned long long* ctr;      // [n_ent] counters in scan order
  const unsigned long long* skey;  // [n_ent] sorted keys
  const uint32_t* sidx;         // [n_ent] and their scan positions
  uint32_t* s_actor;            // [n_ent] actor id of sorted entry e
  unsigned long long* s_ctr;    // [n_ent] its counter
  // sizes and the encoder
  uint32_t opf, n_ops;
  uint32_t* olen;               // [n_ops + 1] op byte lengths, olen[n_ops] = 0
  const uint32_t* ooff;         // [n_ops + 1] their exclusive sums
  OpFileLayout L;               // n_files = ceil(n_ops / opf); sized by launch_opfile_sizes
  uint32_t head[7];             // the 26 constant bytes of an op: [0, 17) up to the map header,
                                // [17, 26) a7 "members" 91
};

// first[handle of members[i]] = min(.., i), hnd[i]; then one scan of the pair table: cnt / ebytes
// of the representatives (cnt, ebytes zeroed beforehand); then rep, keep and the totals
hipError_t launch_rm_mark(hipStream_t s, const RmArgs& a);
hipError_t launch_rm_count(hipStream_t s, const RmArgs& a);
hipError_t launch_rm_keep(hipStream_t s, const RmArgs& a);
// first[] all ones again (the handles of hnd)
hipError_t launch_rm_unmark(hipStream_t s, const RmArgs& a);
// op_pos from kpos
hipError_t launch_rm_scatter(hipStream_t s, const RmArgs& a);
// the second scan of the pair table: key / idx / ctr of every live pair of a marked handle
// (tot[kRmTotGather] counts them); after the sort, s_actor / s_ctr
hipError_t launch_rm_gather(hipStream_t s, const RmArgs& a);
hipError_t launch_rm_entries(hipStream_t s, const RmArgs& a);
hipError_t launch_rm_op_sizes(hipStream_t s, const RmArgs& a);
// the clear texts and the seal's two offset columns.  grid_cap: the most blocks (0: the default)
hipError_t launch_rm_encode(hipStream_t s, const RmArgs& a, uint32_t grid_cap);

// The fold's removal columns of this call, in place: one removal a position of the column (n of
// them), removal i listing members[i] under the entries of representative i -- cnt[i] of them
// from ebeg[i], so a position that is not its member's first, or whose member is absent or dead,
// carries the empty clock and kills nothing.  Zero adds.
struct RmCols {
  const unsigned long long* members;
  uint32_t n, n_ent;
  const uint32_t* ebeg;           // [n + 1]
  const uint32_t* s_actor;
  const unsigned long long* s_ctr;
  uint32_t* add_mbeg;             // [1] = 0
  uint32_t* rm_cbeg;              // [n + 1]
  uint32_t* rm_mbeg;              // [n + 1], rm_mbeg[i] = i
  uint32_t* rmc_actor;
  unsigned long long* rmc_ctr;
  unsigned long long* rm_mem;
};
hipError_t launch_rm_cols(hipStream_t s, const RmCols& a);

}  // namespace ce
