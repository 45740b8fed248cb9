// ce_gset.h -- GSet<u64> (crdts 7: struct GSet<T> { value: BTreeSet<T> }, Op = T): the device
// hash set and its kernels' launch interface (ce_gset.hip), driven by ce_gset_host.cpp.
//
// Table: open addressing over u64 keys, linear probing, capacity a power of two.  An empty slot
// holds 0; the member 0 is held out of band (meta[kGsZero]).  A probe that finds its key does no
// atomic; a probe that reaches an empty slot reserves one unit of the live count, then claims the
// slot with a 64-bit CAS.  The count never passes `limit` (half the capacity), so a probe always
// ends at the key or at an empty slot; a reservation that would pass it raises meta[kGsOverflow]
// instead, and the host grows the table and runs the launch again (inserts are idempotent).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_kernels.h"
#include "ce_opfile.h"

namespace ce {

static constexpr int kGsCount = 0;     // claimed slots (the member 0 not counted)
static constexpr int kGsZero = 1;      // the member 0 is in the set
static constexpr int kGsOverflow = 2;  // an insert was refused at the load bound
static constexpr int kGsMetaWords = 4;

struct GsTable {
  unsigned long long* slots;  // [mask + 1]
  uint32_t mask;
  uint32_t limit;             // claims allowed: (mask + 1) / 2
  uint32_t* meta;             // kGsMetaWords words
};

struct GsDecodeArgs {
  const uint8_t* pt;          // plaintext blob (FileParams.out_off / len)
  const FileParams* params;
  int32_t* status;
  uint32_t n;
  const uint8_t* supported;   // n_supported * 16 bytes
  uint32_t n_supported;
  const uint8_t* apply;       // 1 = insert this file's members (version gate)
  const uint8_t* only;        // null, or per file: decode only files with only[i] != 0
  int large_only;             // only files of more than one page (the fused open took the others)
  GsTable committed;          // probed read-only
  GsTable batch;              // members absent from `committed` are claimed here
  uint32_t* paths;            // [0] files of one element width, [1] files of the general path
};

// what the fused open's GSet grammar (ce_fused.hip k_open_fold_v3<false, true, false, true>) reads
// through DecodeArgs.gs (device memory): the two tables, and the launch's file counts
// paths[0] uniform, [1] general (shared with k_decode_gset), [2] files decoded in the open
struct GsFused {
  GsTable committed, batch;
  uint32_t* paths;
};

// one wave per file: data version, array header, the uniform-width or the general path; statuses
// CE_ERR_PT_LEN / CE_ERR_PT_VERSION / CE_ERR_DECODE into a.status
hipError_t launch_decode_gset(hipStream_t s, const GsDecodeArgs& a, uint32_t grid_waves);
// keys[0..n) into t (a state file's members, local ops)
hipError_t launch_gs_insert(hipStream_t s, GsTable t, const unsigned long long* keys, uint32_t n);
// k <= kGsMaxParts columns (other ranks' pending members) for one launch: part[i] holds
// pre[i + 1] - pre[i] keys, pre[0] = 0, pre[k] = their total (<= 2^31)
static constexpr uint32_t kGsMaxParts = 64;
struct GsParts {
  const unsigned long long* part[kGsMaxParts];
  uint32_t pre[kGsMaxParts + 1];
  uint32_t k;
};
// every key of every part into t, one launch
hipError_t launch_gs_insert_parts(hipStream_t s, GsTable t, const GsParts& ps);
// The state-file reader (a StateWrapper's `value` array in HBM).  One descriptor per file, offsets
// from the launch's base pointer; count < 2^29 and blen < 2^32 (the host sends other files to its
// own parser).  runs: kGsStateRunWords words per file, [0, 5) the lengths of the fixint, cc, cd, ce
// and cf runs, every word 0xffffffff before the first phase.
struct GsStateFile {
  unsigned long long body;  // the first element's byte
  uint32_t blen;            // bytes from there to the end of the file's plaintext
  uint32_t count;           // the array header's count
  uint32_t pre;             // (insert) members of the launch's files before this one
  uint32_t pad;
};
static constexpr uint32_t kGsStateRunWords = 8;
static constexpr uint32_t kGsStateMaxFiles = 128;  // files of one insert launch
// the five phases of k_gs_state_runs over n files, back to back (max_count: the largest count)
hipError_t launch_gs_state_runs(hipStream_t s, const uint8_t* base, const GsStateFile* files, uint32_t n,
                                uint32_t max_count, uint32_t* runs);
// the members of k <= kGsStateMaxFiles files whose runs sum to their count (count 0: skipped) into
// t, total = their members (<= 2^31); runs: the first of these files' words
hipError_t launch_gs_state_insert(hipStream_t s, GsTable t, const uint8_t* base, const GsStateFile* files, uint32_t k,
                                  uint32_t total, const uint32_t* runs);
// every member of src into dst (the batch's commit, and a growth's rehash)
hipError_t launch_gs_move(hipStream_t s, GsTable src, GsTable dst);
// GSet::contains(q[i]) against t for i < n: out[i] = 1 or 0 (k_gs_contains: a grid-stride loop,
// several probes in flight per lane).  grid_cap: the most blocks to launch (0: 2048)
hipError_t launch_gs_contains(hipStream_t s, GsTable t, const unsigned long long* q, uint64_t n, uint8_t* out,
                              uint32_t grid_cap);
// the live members of t, in no order, into out[0..*n_out) (*n_out zero before the launch)
hipError_t launch_gs_collect(hipStream_t s, GsTable t, unsigned long long* out, uint32_t* n_out);
// the serializer over the sorted members v[0..n): w[i] = element i's encoded length (1, 2, 3, 5
// or 9); then, with off = the exclusive scan of w, element i written at out[off[i]] and the clear
// length head_len + off[n - 1] + w[n - 1] at clear_len_at (the seal's offs[1])
hipError_t launch_gs_widths(hipStream_t s, const unsigned long long* v, uint32_t n, uint32_t* w);
hipError_t launch_gs_write(hipStream_t s, const unsigned long long* v, const uint32_t* off, uint32_t n, uint8_t* out,
                           unsigned long long* clear_len_at, uint64_t head_len);

// ---- the op-file writer (ce_gset_write.hip): a member column cut into files of per_file members
// (the last may be shorter), file i's clear text = data version || array header || its members,
// each in its smallest form.  per_file <= kGsFileMembers, so a clear text is at most one page.
static constexpr uint32_t kGsFileMembers = 453;  // cf members whose clear text fills a 4096-byte page
struct GsFilesArgs {
  const unsigned long long* members;  // [n]
  unsigned long long n;
  uint32_t per_file;
  OpFileLayout L;              // n_files = ceil(n / per_file) > 0 (ce_opfile.h)
};
hipError_t launch_gs_file_sizes(hipStream_t s, const GsFilesArgs& a);
// grid_cap: the most blocks to launch (0: the default)
hipError_t launch_gs_files_encode(hipStream_t s, const GsFilesArgs& a, uint32_t grid_cap);
// CE_GSET_APPLY_NEW_ONLY over the sorted column s[0..n): keep[i] = 1 where s[i] is the first of
// its run and t does not hold it, keep[n] = 0; then, with pos = the exclusive scan of keep over
// n + 1 words, the kept members in order into out (pos[n] of them)
hipError_t launch_gs_new_mark(hipStream_t s, GsTable t, const unsigned long long* sorted, uint32_t n, uint32_t* keep);
hipError_t launch_gs_new_compact(hipStream_t s, const unsigned long long* sorted, const uint32_t* keep,
                                 const uint32_t* pos, uint32_t n, unsigned long long* out);

}  // namespace ce
