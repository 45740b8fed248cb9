// ce_orswot_write.h -- the Orswot add-op writer's launch interface (ce_orswot_write.hip), driven by
// ds_add_members_device (ce_dotset_host.cpp).
//
// A member column in HBM is cut, in order, into Add ops of per_op members (the last may be
// shorter) and the ops into files of ops_per_file ops (the last may hold fewer).  Op j of the call
// is Add { dot: Dot { actor: local, counter: c0 + 1 + j }, members }; file i's clear text is
//   data version (16) || Vec header || its ops, each
//   81 a3 "Add" 82 a3 "dot" 82 a5 "actor" c4 10 <actor> a7 "counter" <counter> a7 "members"
//   <array header> <members>
// with every integer in its smallest unsigned form: 51 + w(counter) + h(count) + sum w(member)
// bytes an op.  The host admits only (per_op, ops_per_file) pairs whose worst case is one page.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_opfile.h"

namespace ce {

static constexpr uint32_t kOwPage = 4096;      // the longest clear text of a file
static constexpr uint32_t kOwHeadBytes = 43;   // an op up to its counter
static constexpr uint32_t kOwFixedBytes = 51;  // ... and the a7 "members" behind the counter
// ops of fewer members than this are sized and encoded a lane per op, longer ones a 16-lane
// group per op (the members' array header changes form at the same count)
static constexpr uint32_t kOwGroupOps = 16;

// an op's worst case: a 9-byte counter and 9-byte members
CE_HD constexpr uint64_t ow_op_bound(uint64_t cnt) { return kOwFixedBytes + 9 + arr_hdr_len((uint32_t)cnt) + 9 * cnt; }
// a file's worst case; the one-page rule is ow_file_bound(ops_per_file, per_op) <= kOwPage
CE_HD constexpr uint64_t ow_file_bound(uint64_t ops, uint64_t per_op) {
  return 16 + arr_hdr_len((uint32_t)(ops > 65535 ? 65535 : ops)) + ops * ow_op_bound(per_op);
}

struct OwArgs {
  const unsigned long long* members;  // [n]
  unsigned long long n;
  unsigned long long c0;       // the local actor's counter before the call: op j carries c0 + 1 + j
  uint32_t per_op, opf;        // members an op, ops a file
  uint32_t n_ops;              // ceil(n / per_op) > 0
  uint32_t* olen;              // [n_ops + 1] op byte lengths, olen[n_ops] = 0 (the op size pass)
  const uint32_t* ooff;        // [n_ops + 1] their exclusive sums
  OpFileLayout L;              // n_files = ceil(n_ops / opf); sized by launch_opfile_sizes
  // the per-call constant of every op: bytes [0, 43) the op up to its counter (the local actor
  // inside), bytes [43, 51) a7 "members", one pad byte
  uint32_t head[13];
};

// olen[j] for every op, olen[n_ops] = 0
hipError_t launch_ow_op_sizes(hipStream_t s, const OwArgs& a);
// the clear texts, and the seal's two offset columns.  grid_cap: the most blocks (0: the default)
hipError_t launch_ow_encode(hipStream_t s, const OwArgs& a, uint32_t grid_cap);

// The fold's add columns of this call, in place.  Add k covers the `span` members from k * span:
// span = per_op gives one add an op (add_mbeg[j] = j * per_op); span = 1 gives one add a member,
// the members of an op sharing its counter -- the same entries and clock, in the form the fold's
// kernels are built for (a lane an add).  One run of one actor whose counters never fall and
// start above the clock's, so every add is applied and add k's exclusive maximum is its
// predecessor's counter (0 for the first): the form k_ds_contig leaves for the sort-free fold.
// Zero removals.
struct OwCols {
  const unsigned long long* members;
  unsigned long long n, c0;
  uint32_t per_op, span;
  uint32_t n_add;              // ceil(n / span)
  uint32_t actor_id;
  uint32_t* add_actor;
  unsigned long long* add_ctr;
  uint32_t* add_mbeg;          // [n_add + 1], the sentinel n
  unsigned long long* add_mem;
  uint32_t* rm_cbeg;           // [1] = 0
  uint32_t* rm_mbeg;           // [1] = 0
  uint8_t* applied;
  unsigned long long* excl;
};
hipError_t launch_ow_cols(hipStream_t s, const OwCols& a);

}  // namespace ce
