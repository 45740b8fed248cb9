// ce_core.h -- the Core object (crdt-enc/src/lib.rs:188-207 Core / CoreMutData) and the host
// helpers shared by ce_core.cpp (VClock / GCounter state) and ce_dotset_host.cpp (Orswot / MVReg).
#pragma once
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "ce_internal.h"
#include "ce_opfile.h"

namespace ce {
int storage_load_ops_vec(ce_storage* s, const std::vector<Uuid>& actors,
                         const std::vector<uint64_t>& first, std::vector<uint8_t>* blob,
                         std::vector<uint64_t>* offs, std::vector<uint32_t>* aidx,
                         std::vector<uint64_t>* vers);
int storage_list_op_actors_vec(ce_storage* s, std::vector<Uuid>* out);
int storage_list_states_vec(ce_storage* s, std::vector<std::string>* out);
int storage_read_state(ce_storage* s, const std::string& name, std::vector<uint8_t>* out);
int storage_store_content(ce_storage* s, const char* sub, const uint8_t* d, size_t n,
                          std::string* name);
int storage_remove_state(ce_storage* s, const std::string& name);
int storage_store_op(ce_storage* s, const Uuid& actor, uint64_t version, const uint8_t* d,
                     size_t n);
int storage_remove_op(ce_storage* s, const Uuid& actor, uint64_t version);
int storage_load_local_meta(ce_storage* s, std::vector<uint8_t>* out, bool* missing);
int storage_store_local_meta(ce_storage* s, const uint8_t* d, size_t n);
ce_storage* storage_new(const std::string& local, const std::string& remote);

struct DsState;  // Orswot / MVReg state (ce_dotset_host.cpp)
void ds_free(DsState* d);
struct GsState;  // GSet<u64> state: the device hash set (ce_gset_host.cpp)
void gs_free(GsState* g);
struct LwState;  // LWWReg<u64, u64> state: the register and the ingest's record column (ce_lww_host.cpp)
void lw_free(LwState* l);

inline bool is_dotset_kind(int kind) { return kind == CE_STATE_ORSWOT || kind == CE_STATE_MVREG; }
// kinds the dense multi-GPU calls refuse (export / import / the generic sharded ingest and pending
// batch): whole states travel as state bytes, and GSet, PNCounter and LWWReg have sharded-ingest
// entry points of their own (ce_core_gset_*, ce_core_pn_*, ce_core_lwwreg_*)
inline bool no_dense_exchange(int kind) {
  return is_dotset_kind(kind) || kind == CE_STATE_PNCOUNTER || kind == CE_STATE_GSET || kind == CE_STATE_LWWREG;
}
// planes of the dense state and batch (u64[planes * cap]): PNCounter keeps p at [slot] and n at
// [slot + cap]; next_op_versions is one plane for every kind
inline uint32_t state_planes(int kind) { return kind == CE_STATE_PNCOUNTER ? 2u : 1u; }
}  // namespace ce

namespace ce {
struct AltKey {  // a key of the set besides the latest (ce_core_set_keys, CE_OPEN_MULTI_KEY)
  uint8_t version[16];
  std::vector<uint8_t> key;
};
}  // namespace ce

struct ce_core {
  ce_ctx* ctx = nullptr;
  int kind = CE_STATE_GCOUNTER;
  std::vector<ce::Uuid> supported;  // sorted (lib.rs:227-228)
  ce::Uuid current_data_version{};
  ce_storage* storage = nullptr;
  uint32_t flags = 0;
  ce::Uuid local_actor{};
  bool has_key = false;
  uint8_t key_version[16] = {0};
  std::vector<uint8_t> key;
  std::vector<ce::AltKey> alt_keys;  // tried in id order on AUTH failures (CE_OPEN_MULTI_KEY)
  std::map<std::string, uint64_t> path_counts;  // which code path ran (ce_core_path_count)
  // actor table: UUID -> hash slot; ActorSlot.pad[0] holds the actor's stable id (insertion
  // order, survives table growth) used by the dot-set kinds' device arrays.
  uint32_t cap = 0, size = 0, registered = 0;
  std::vector<ce::ActorSlot> h_table;
  std::vector<ce::Uuid> slot_actor;
  std::vector<ce::Uuid> id_actor;   // stable id -> UUID
  std::vector<uint64_t> nov;  // next_op_versions by slot
  std::unordered_map<ce::Uuid, uint32_t, ce::UuidHash> slot_of;
  bool table_dirty = true;
  uint64_t table_gen = 0;               // bumped whenever an actor gets a slot or slots move
  std::vector<uint8_t> ser_buf, file_buf;  // compaction: serialized state, sealed file (reused)
  // compact_into: the caller's buffer; a compaction that fits writes the file there directly
  // (sink_len = its length) instead of into file_buf
  uint8_t* sink = nullptr;
  size_t sink_cap = 0, sink_len = 0;
  // ce_core_compact_into_async: the sealed file's download into the sink is left in flight on
  // copy_stream (ticket -> copy_ev[ticket % kAsyncSlots]); the next compaction's seal waits for
  // the last one on the device before it rewrites the sealed output
  static constexpr uint32_t kAsyncSlots = 16;
  bool sink_async = false;
  uint64_t sink_ticket = 0;               // set by the device writer when it left a copy in flight
  hipStream_t copy_stream = nullptr;
  hipEvent_t copy_ev[kAsyncSlots] = {};
  uint64_t copy_slot_ticket[kAsyncSlots] = {};
  uint64_t copy_next = 0;                 // last ticket handed out
  // pinned, mapped: per slot, the sealed file's length the device wrote behind the seal
  // (ce_core_compact_wait); the download itself is enqueued by ds_async_kick once the seal is
  // done (the runtime's DMA copy needs the exact length on the host), at most one pending
  ce::HostBuf copy_len;
  uint64_t* copy_len_dev = nullptr;
  hipEvent_t seal_ev = nullptr;
  // the download on an SDMA engine when the HSA runtime offers one (copy_sig per slot), else the
  // HIP runtime's copy on copy_stream (copy_ev); copy_last_slot: the newest download's slot
  ce::DmaD2H dma;
  bool dma_tried = false;
  hsa_signal_t copy_sig[kAsyncSlots] = {};
  bool copy_dma[kAsyncSlots] = {};
  int copy_last_slot = -1;
  bool pend = false;
  uint32_t pend_slot = 0;
  uint8_t* pend_dst = nullptr;
  std::vector<uint32_t> sorted_slots;   // used slots in UUID byte order (BTreeMap order)
  uint64_t sorted_gen = ~0ull;
  std::vector<uint8_t> last_writers;    // writer list of the previous ingest and its slots
  std::vector<uint32_t> last_wslot;
  uint64_t last_writers_gen = ~0ull;
  ce::DevBuf d_table, d_state, d_batch, d_supported, d_refold2, d_tmp, d_gate, d_meta;
  ce::DevBuf d_sorted, d_wslot;                  // sorted_slots on the device (compaction serializer)
  uint64_t d_sorted_gen = ~0ull;
  int files_per_wave = 4;  // fused kernel geometry (CE_FILES_PER_WAVE overrides)
  bool supported_on_device = false;
  bool host_compact = false;  // CE_HOST_COMPACT=1: serialize on the host (reference check)
  int fused = 2;           // fused kernel: 1 keystream staged in LDS, 2 block-owning lanes (CE_FUSED)
  std::set<std::string> read_states;  // lib.rs:205
  ce_ctx* aux = nullptr;              // single-file work during a batch (exotic envelopes)
  ce::DsState* ds = nullptr;          // Orswot / MVReg state (dot-set kinds only)
  ce::GsState* gs = nullptr;          // GSet state (CE_STATE_GSET only)
  ce::LwState* lw = nullptr;          // LWWReg state (CE_STATE_LWWREG only)
  // sharded ingest (ce_core_ingest_ops_device_sharded): the batch is folded into d_batch and
  // held there with its next_op_versions until ce_core_pending_commit
  bool pending = false;
  uint64_t pending_gen = 0;                                  // table_gen of the pending batch
  std::vector<std::pair<ce::Uuid, uint64_t>> pending_nov;    // (writer, next_op_version)
  ce::DevBuf d_shard;                  // writer UUIDs | e0 | stats scratch (ce_core_shard_*)
  ce::HostBuf h_shard;                 // pinned staging of the e0 upload (its own: the copy is async)
  std::vector<uint64_t> shard_e0;      // the e0 d_shard holds
  std::vector<uint8_t> shard_writers;  // the writer list d_shard holds
  // with_state reads: the host-buffer forms' query / answer columns, the dense kinds' sums and
  // gather indices (device), and the pinned block their small results land in
  ce::DevBuf d_rq, d_ra, d_rsum;
  ce::HostBuf h_read;
};

namespace ce {
// the open kernels ctx's launchers took since the last call -> c's path counts
inline void count_open_launches(ce_core* c, ce_ctx* ctx) {
  for (uint32_t i = 0; i < ctx->open_log.n; i++) c->path_counts[ctx->open_log.took[i]]++;
  ctx->open_log.n = 0;
}
}  // namespace ce

namespace ce {

// msgpack writer (rmp-serde to_vec_named)
struct Wr {
  std::vector<uint8_t> b;
  void u8(uint8_t v) { b.push_back(v); }
  void be(uint64_t v, int k) {
    for (int j = k - 1; j >= 0; j--) b.push_back((uint8_t)(v >> (8 * j)));
  }
  void uint(uint64_t v) {
    if (v <= 0x7f) u8((uint8_t)v);
    else if (v <= 0xff) { u8(0xcc); be(v, 1); }
    else if (v <= 0xffff) { u8(0xcd); be(v, 2); }
    else if (v <= 0xffffffffull) { u8(0xce); be(v, 4); }
    else { u8(0xcf); be(v, 8); }
  }
  void str(const char* s) {
    const size_t l = std::strlen(s);
    u8((uint8_t)(0xa0 | l));
    b.insert(b.end(), s, s + l);
  }
  void bin(const uint8_t* d, size_t l) {
    if (l <= 0xff) { u8(0xc4); be(l, 1); }
    else if (l <= 0xffff) { u8(0xc5); be(l, 2); }
    else { u8(0xc6); be(l, 4); }
    b.insert(b.end(), d, d + l);
  }
  void map(size_t n) {
    if (n <= 15) u8((uint8_t)(0x80 | n));
    else if (n <= 0xffff) { u8(0xde); be(n, 2); }
    else { u8(0xdf); be(n, 4); }
  }
  void arr(size_t n) {
    if (n <= 15) u8((uint8_t)(0x90 | n));
    else if (n <= 0xffff) { u8(0xdc); be(n, 2); }
    else { u8(0xdd); be(n, 4); }
  }
};

using Dots = std::vector<std::pair<Uuid, uint64_t>>;

// CE_HOST_PROF=1: wall time of host phases to stderr (diagnostics only)
struct HostPhase {
  const char* name;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit HostPhase(const char* n) : name(n) {}
  ~HostPhase() {
    static const bool on = std::getenv("CE_HOST_PROF") != nullptr;
    if (!on || !name || !*name) return;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "CE_HOST_PROF %-24s %9.3f ms\n", name, ms);
  }
};

// next_op_versions of an ingest whose device commit is still in flight (compact_enqueue)
struct NovApply {
  const uint32_t* wslot;                 // device: slot of each writer
  const unsigned long long* newnov;      // device: the gate's next_op_versions per writer
  uint32_t m;
  const uint32_t* counters;              // device: the ingest's counter block
  unsigned long long* nov_dev = nullptr; // device: the pre-ingest next_op_versions (cap words),
                                         // uploaded with the gate block; the compaction applies
                                         // newnov to it in place
  const uint8_t* host_tail = nullptr;    // out (set by the compaction): pinned host copy of
                                         // [clear length | the counters | newnov[m]] after sync
  // the ingest's commit (k_merge_max_if: state = max(state, batch) over merge_n words), left to
  // the compaction's first kernel when set: one launch and one dependency gap fewer
  unsigned long long* merge_dst = nullptr;
  const unsigned long long* merge_src = nullptr;
  uint32_t merge_n = 0;
};

bool skip_any(Rd& r, int depth = 0);
bool bytes_any(Rd& r, std::vector<uint8_t>* out);
bool read_struct(Rd& r, const std::vector<const char*>& names,
                 const std::function<bool(int, Rd&)>& cb);
bool read_vclock(Rd& r, Dots* out);
int insert_actor(ce_core* c, const Uuid& u, uint32_t* slot);
// slots of m actors (16 bytes each) after a table growth moved the ones handed out before it
void refresh_slots(ce_core* c, const uint8_t* actors, uint32_t m, std::vector<uint32_t>* slots);
inline uint32_t actor_id_of_slot(const ce_core* c, uint32_t slot) { return c->h_table[slot].pad[0]; }
int table_upload(ce_core* c);
KeyRef key_of(ce_core* c);
int ensure_supported(ce_core* c);
int resolve_host_parse(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                       bool outer);
uint32_t host_gate(const uint32_t* fa, const uint64_t* fv, uint32_t n, std::vector<uint64_t>* expect,
                   uint8_t* apply);
// neg (PNCounter): the dots of the n plane, merged in the same launch
int merge_dots_host(ce_core* c, const Dots& dots, const Dots* neg = nullptr);
// read_remote_ops over a batch resident in HBM (ce_core.cpp).  shard_hi (device, m + 1 words):
// the sharded gate's windows and flags (ce_shard.hip) instead of the local gate; the batch is
// then left pending (not committed) for ce_core_pending_commit.
int ingest_ops_dev_sharded(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                           uint64_t blob_len, const uint8_t* actors, uint32_t m, const uint32_t* d_fa,
                           const uint64_t* d_fv, const uint64_t* shard_hi, int32_t* status_out);

// Shared by the kinds' own sharded ingests (ce_shard_host.cpp).
// next_op_versions.get(writer) of m writers (16 bytes each), 0 for one without a slot
void writer_versions_of(const ce_core* c, const uint8_t* actors, uint32_t m, std::vector<uint64_t>* e0);
// The sharded gate on the device: apply[i] = expect[writer] <= version < d_hi[writer]
// (k_gate_window over the windows every rank agreed on, into ctx->apply).  gate: the caller's
// scratch for e0 u64[m] | newnov u64[m].  The host reads back the m window ends and the flags
// word, no per-file metadata: expect[a] = max(expect[a], hi[a]), *gap = the windows stop at a gap.
// CE_ERR_SHARD (flags kShardBad / kShardE0Mismatch): nothing may be opened or folded.
int shard_gate_window(ce_core* c, DevBuf* gate, uint32_t n, uint32_t m, const uint32_t* d_fa,
                      const uint64_t* d_fv, const uint64_t* d_hi, std::vector<uint64_t>* expect, bool* gap);
// a pending batch's next_op_versions (c->pending_nov, lib.rs:537-538) into the table, uploaded
int commit_pending_nov(ce_core* c);

// dot-set kinds (ce_dotset_host.cpp): same contracts as the VClock/GCounter paths in ce_core.cpp
int ds_init(ce_core* c);
int ds_reset(ce_core* c);
int ds_ingest_ops(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                  uint64_t blob_len, const uint8_t* actors, uint32_t m, const uint32_t* d_fa,
                  const uint64_t* d_fv, int32_t* status_out);
// read_remote_states after load_states; plaintext StateWrappers (after the data version)
// sws[i] = {nullptr, 0} for files whose status st[i] is already a failure.
int ds_compact_device(ce_core* c, ce_ctx* x, const uint8_t* outer, const uint8_t* prefix16,
                      const uint8_t* nonce, const KeyRef& key, std::vector<uint8_t>* file);
int ds_merge_states_device(ce_core* c, const uint8_t* out, const std::vector<uint64_t>& off,
                           const std::vector<uint64_t>& len, int32_t* st, int32_t* status_out);
int ds_merge_states(ce_core* c, const std::vector<std::pair<const uint8_t*, size_t>>& sws,
                    int32_t* st, int32_t* status_out);
int ds_serialize(ce_core* c, std::vector<uint8_t>* out);
// Orswot: the same bytes written on the device into dst (cap bytes); *len = their length
// compact_into_async: enqueue the pending download once its seal is done (force: wait for it)
int ds_async_kick(ce_core* c, bool force);
// the newest compaction download done reading seal_out (host wait, or ordered on s)
int ds_download_fence(ce_core* c, hipStream_t s, bool device);
// the last fold's / k-way merge's closing counts and deferred set (waits for the stream)
int ds_settle(ce_core* c);
int ds_state_bytes_device(ce_core* c, ce_ctx* x, uint8_t* dst, uint64_t cap, uint64_t* len);
int ds_export_columns_device(ce_core* c, uint8_t* dst, uint64_t cap, uint64_t* len);
int ds_merge_columns_device(ce_core* c, const uint8_t* const* parts, const uint64_t* lens, uint32_t k);
// with_state reads (lib.rs:325-330), each after ds_settle.  Orswot: contains / len / members from
// the per-handle live flags (rebuilt when the tables changed since), entries[m] per queried member
// (u32 beg[n + 1], padded to 8 bytes, then 24-byte (uuid, u64 LE) entries in UUID order).  Orswot
// and MVReg: the clock / the join of the values' clocks, counters > 0, in no order.  MVReg: the
// values in ds_serialize's order.
int ds_contains_device(ce_core* c, const uint64_t* d_members, uint64_t n, uint8_t* d_out);
int ds_set_len(ce_core* c, uint64_t* n);
int ds_members_device(ce_core* c, uint64_t* d_dst, uint64_t cap, uint64_t* n);
int ds_read_clock(ce_core* c, Dots* out);
int ds_member_clocks(ce_core* c, const uint64_t* members, uint32_t n, std::vector<uint8_t>* out);
int ds_mvreg_read(ce_core* c, std::vector<uint64_t>* out);
// Core::apply_ops for a local Vec<S::Op> (already validated by ds_check_ops)
int ds_check_ops(ce_core* c, const uint8_t* ops, size_t len);
int ds_apply_local_ops(ce_core* c, const uint8_t* ops, size_t len);
// The Orswot add-op writer (ce_core_orswot_add_members[_device]): Core::apply_ops over a member
// column cut into Add ops of per_op members by the local actor, ops_per_file ops a file.
// ow_shape: the normalised pair (per_op 0: 1; ops_per_file 0: 28 at one member an op, else the
// most the page allows) and the worst-case sizes; false when a file may pass one page or the files
// do not fit a u32.  ds_add_check: everything either form refuses from its arguments alone.
struct OwShape {
  uint32_t per_op, opf;
  uint64_t n_ops;
  uint32_t files;
  uint64_t bytes, clear;  // the sealed files' and the clear texts' worst case
};
bool ow_shape(uint64_t n, uint32_t per_op, uint32_t ops_per_file, OwShape* o);
int ds_add_check(ce_core* c, uint64_t n, uint32_t per_op, uint32_t ops_per_file, uint32_t flags, OwShape* o);
// the arguments have passed ds_add_check and d_files holds sh.bytes: reads the local actor's
// counter (refusing a call that would pass 2^64 - 1), then sized, encoded and sealed on the device
// into d_files / d_file_offs, then stored, folded and bumped
int ds_add_members_device(ce_core* c, const uint64_t* d_members, uint64_t n, const OwShape& sh, const uint8_t* nonces,
                          uint8_t* d_files, uint64_t* d_file_offs, uint32_t* n_files, uint64_t* bytes);
// the same over a host column: the files and their n_files + 1 offsets come back to the host
int ds_add_members_host(ce_core* c, const uint64_t* members, uint64_t n, const OwShape& sh, const uint8_t* nonces,
                        std::vector<uint8_t>* files, std::vector<uint64_t>* file_offs, uint32_t* n_files);
// The Orswot Rm-op writer (ce_core_orswot_rm_members[_device]): one Rm op a member of the column,
// its clock the member's entries in the committed state.  ds_rm_check: everything either form
// refuses from its arguments alone.  ds_rm_members_device: d_files null is the sizing call (the
// exact n_ops / n_files / bytes, nothing written or changed); else cap is checked against the
// exact bytes behind the size passes, before the seal.
int ds_rm_check(ce_core* c, uint64_t n, uint32_t ops_per_file, uint32_t flags);
int ds_rm_members_device(ce_core* c, const uint64_t* d_members, uint64_t n, uint32_t ops_per_file, uint32_t flags,
                         const uint8_t* nonces, uint8_t* d_files, uint64_t cap, uint64_t* d_file_offs, uint64_t* n_ops,
                         uint32_t* n_files, uint64_t* bytes);
int ds_rm_members_host(ce_core* c, const uint64_t* members, uint64_t n, uint32_t ops_per_file, uint32_t flags,
                       const uint8_t* nonces, std::vector<uint8_t>* out, std::vector<uint64_t>* fo, uint32_t* n_files);

// GSet<u64> (ce_gset_host.cpp): the members live in a device hash set; next_op_versions, the
// actor table and the storage plumbing are ce_core.cpp's, as for every kind
int gs_init(ce_core* c);
int gs_reset(ce_core* c);
int gs_settle(ce_core* c);
int gs_ingest_ops(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                  uint64_t blob_len, const uint8_t* actors, uint32_t m, const uint32_t* d_fa,
                  const uint64_t* d_fv, int32_t* status_out);
// members (a state file's `value`, a local Vec<u64>) into the committed set
int gs_insert_members(ce_core* c, const std::vector<uint64_t>& members);
// the set in BTreeSet order: collected and sorted on the device
int gs_members_sorted(ce_core* c, std::vector<uint64_t>* out);
// the device writer.  head: the clear text up to and including a5"state" (an ingest-format
// compaction's data version, next_op_versions); the members are collected, sorted, sized,
// scanned and written after it on the device.  gs_serialize_device downloads the clear text;
// gs_compact_device seals it there (file = outer || Cryptor::encrypt(clear)) and downloads the file
int gs_serialize_device(ce_core* c, std::vector<uint8_t> head, std::vector<uint8_t>* out);
int gs_compact_device(ce_core* c, std::vector<uint8_t> head, const uint8_t* outer, const uint8_t* nonce,
                      const KeyRef& key, std::vector<uint8_t>* file);
// gs_serialize_device's bytes left in HBM and copied device to device into d_dst (cap bytes);
// *len = their length, also when cap is too small (CE_ERR_INVALID_ARG, d_dst untouched)
int gs_state_bytes_device(ce_core* c, std::vector<uint8_t> head, uint8_t* d_dst, uint64_t cap, uint64_t* len);
// read_remote_states over StateWrapper plaintexts in HBM (file i at base + off[i], len[i] bytes,
// st[i] its status so far): heads on the host, canonical bodies decoded and inserted on the
// device, every other file through the host parser; all or nothing
int gs_merge_states_device(ce_core* c, const uint8_t* base, const std::vector<uint64_t>& off,
                           const std::vector<uint64_t>& len, int32_t* st, int32_t* status_out);
// with_state reads (lib.rs:325-330) of the committed table (a pending sharded batch is no part of
// them): contains over a query column in HBM, the member count, the members ascending in HBM
// (*n always the count; nothing written when cap < *n)
int gs_contains_device(ce_core* c, const uint64_t* d_members, uint64_t n, uint8_t* d_out);
int gs_set_len(ce_core* c, uint64_t* n);
int gs_members_device(ce_core* c, uint64_t* d_dst, uint64_t cap, uint64_t* n);
// Core::apply_ops over a member column in HBM cut into files of per_file members
// (ce_core_gset_apply_members_device, whose refusals the caller has checked): sized, encoded and
// sealed on the device into d_files / d_file_offs, then stored, inserted and bumped
int gs_apply_members_device(ce_core* c, const uint64_t* d_members, uint64_t n, uint32_t per_file, uint32_t flags,
                            const uint8_t* nonces, uint8_t* d_files, uint64_t* d_file_offs, uint32_t* n_files,
                            uint64_t* bytes);
// Vec<u64> as rmp-serde reads it (any non-negative integer form); false: CE_ERR_DECODE
bool parse_gset_ops(const uint8_t* p, size_t n, std::vector<uint64_t>* out);
// GSet { value: BTreeSet<u64> }: the reader (any order, duplicates) and the canonical writer
bool read_gset_state(Rd& r, std::vector<uint64_t>* out);
void write_gset_state(Wr* w, const std::vector<uint64_t>& sorted_members);

// The op-file writers' shared host steps (ce_opfile_host.cpp), in a writer's order: carve, stage,
// its own size passes and opfile_scan, its encoder, opfile_seal, opfile_store, its fold,
// opfile_finish.  `who` ("gset apply", "orswot add", "orswot rm") heads the error strings.
// offs and the four u32 columns clen | xlen | coff | xoff, `stride` (> n_files) words apart from
// cols, the sealed offsets' column and the data version into L
void opfile_carve(const ce_core* c, unsigned long long* offs, uint32_t* cols, uint64_t stride, uint64_t* d_file_offs,
                  OpFileLayout* L);
// ctx->blob (U bytes of clear text: L->clear), ctx->nonces and ctx->outer_ver reserved; the nonces
// (null: random ones into *drawn, which must live to the next wait) and kCoreVersion uploaded
int opfile_stage(ce_core* c, const char* who, uint64_t U, const uint8_t* nonces, std::vector<uint8_t>* drawn,
                 OpFileLayout* L);
// clen -> coff and xlen -> xoff over n_files + 1 words; tmp is the writer's own scan scratch
hipError_t opfile_scan(const OpFileLayout& L, void* tmp, size_t tmp_bytes, hipStream_t s);
// device_seal of the clear texts into d_files, then one wait for *total = file_offs[n_files] and,
// with d_word, one more device word
int opfile_seal(ce_core* c, const char* who, const OpFileLayout& L, uint64_t U, uint8_t* d_files, uint64_t* total,
                const unsigned long long* d_word = nullptr, uint64_t* word = nullptr);
// the local actor's slot, *v0 = next_op_versions.get(actor), and with storage the files' download
// and store as versions v0, v0 + 1, ...
int opfile_store(ce_core* c, const char* who, const OpFileLayout& L, const uint8_t* d_files, uint64_t total, uint64_t* v0);
// next_op_versions[local actor] = v0 + F (the slot read again: a growth may have moved it), table_upload
int opfile_finish(ce_core* c, uint64_t v0, uint32_t F);
// nothing to write: the one zero offset (d_file_offs null: none), no file, no version
int opfile_empty(ce_core* c, const char* who, uint64_t* d_file_offs, uint32_t* n_files, uint64_t* bytes);
// the host forms' way back: total bytes of files and F + 1 offsets from the two device buffers
int opfile_download(ce_ctx* ctx, const char* who, const DevBuf& files, const DevBuf& offs, uint64_t total, uint32_t F,
                    std::vector<uint8_t>* out, std::vector<uint64_t>* fo);
// a malloc'd copy for the caller to ce_buf_free; the files and offsets of a host form (either may be null)
void fill_buf(ce_buf* out, const void* p, size_t n);
void fill_files(ce_buf* files, ce_buf* file_offs, const std::vector<uint8_t>& out, const std::vector<uint64_t>& fo);

// LWWReg<u64, u64> (ce_lww_host.cpp): the register lives on the host; next_op_versions, the actor
// table and the storage plumbing are ce_core.cpp's, as for every kind
int lw_init(ce_core* c);
int lw_reset(ce_core* c);
int lw_ingest_ops(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                  uint64_t blob_len, const uint8_t* actors, uint32_t m, const uint32_t* d_fa,
                  const uint64_t* d_fv, int32_t* status_out);
// (val, marker) pairs (state files in call order, a local Vec<LWWReg>) through LWWReg::update
void lw_apply_pairs(ce_core* c, const std::vector<uint64_t>& pairs);
void lw_read(ce_core* c, uint64_t* val, uint64_t* marker);
// Vec<LWWReg> as rmp-serde reads it, as (val, marker) pairs appended to out; false: CE_ERR_DECODE
bool parse_lww_ops(const uint8_t* p, size_t n, std::vector<uint64_t>* out);
// LWWReg { val, marker }: the reader (one pair appended) and the canonical writer
bool read_lww_state(Rd& r, std::vector<uint64_t>* out);
void write_lww_state(ce_core* c, Wr* w);

}  // namespace ce
