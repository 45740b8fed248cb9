// ce_gset_host.cpp -- Core<GSet<u64>> (CE_STATE_GSET): the host side of the device hash set
// (ce_gset.h).  Same contracts as the VClock / GCounter paths in ce_core.cpp.
//
// All-or-nothing (lib.rs:497-514): single-page files are opened, checked and decoded in the fused
// open (ce_fused.hip k_open_fold_v3's GS form, plaintext in LDS); larger files, host-parse
// envelopes, multi-key retries and a refold after the batch table grew go through HBM and
// k_decode_gset.  Both insert the gated files' members into the BATCH table, probing the committed
// table read-only (members already known claim nothing).  The host then reads the statuses: a
// failure clears the batch table and the committed set is untouched; otherwise k_gs_move commits
// the batch table's members.  Growth: a launch that raised the overflow flag is run again after
// the host rehashed the table into twice the capacity (inserts are idempotent).
//
// Sharded (a batch partitioned across ranks by op-file address, at the end of this file): the same
// fold with the ranks' agreed windows as the gate (k_gate_window), after which the batch table
// stays PENDING; the ranks exchange its members as u64 columns (ce_core_gset_pending_members) and
// each commits its own batch table and the others' columns, or every rank drops its batch
// (ce_core_gset_pending_commit).
//
// Written from HBM (ce_core_gset_apply_members[_device]): Core::apply_ops over a member column cut
// into one-page op files, sized and encoded by ce_gset_write.hip, sealed by device_seal into the
// caller's buffer, then stored, inserted into the committed table and counted in next_op_versions.
#include <algorithm>
#include <cstring>

#include "ce_core.h"
#include "ce_dotset.h"
#include "ce_dotset_io.h"
#include "ce_gset.h"

namespace ce {

struct GsState {
  DevBuf slots, bslots;  // committed / batch table
  DevBuf meta;           // u32 words: committed [0,4) | batch [4,8) | rehash [8,12) | paths [12,15) | collect count [15]
  uint32_t cap = 0, bcap = 0;
  bool batch_dirty = false;
  DevBuf col, sorted, vals, sort_tmp, scan_tmp, only;
  DevBuf gate;      // the sharded gate's block: e0 u64[m] | newnov u64[m]
  DevBuf fused;     // GsFused: what the fused open reads through DecodeArgs.gs
  GsFused h_fused;  // its host copy (lives through the upload)
  // the state-file reader: GsStateFile[n] | run words [kGsStateRunWords * n]
  DevBuf rd;
  HostBuf h_rd;                  // pinned: the heads' prefixes, the descriptors' upload, the run table
  uint64_t head_hint = 1u << 14;  // state head prefix to download (gs_merge_states_device)
  // the op-file writer (gs_apply_members_device): per file, u32 clen | xlen | coff | xoff and the
  // seal's u64 clear offsets (n_files + 1 of each); the filter's u32 keep | pos (n + 1 of each);
  // the host twin's uploaded column, sealed files and offsets
  DevBuf wr, filt, up_col, up_files, up_offs;
};

void gs_free(GsState* g) { delete g; }

namespace {

constexpr uint32_t kMetaWords = 16;
constexpr uint32_t kMinCap = 16;

uint32_t pow2_at_least(uint64_t v) {
  uint32_t p = kMinCap;
  while (p < v && p < (1u << 31)) p <<= 1;
  return p;
}

GsTable committed(const GsState* g) {
  return GsTable{g->slots.as<unsigned long long>(), g->cap - 1, g->cap / 2, g->meta.as<uint32_t>()};
}
GsTable batch(const GsState* g) {
  return GsTable{g->bslots.as<unsigned long long>(), g->bcap - 1, g->bcap / 2, g->meta.as<uint32_t>() + 4};
}

int read_meta(ce_core* c, uint32_t* hm) {
  hipError_t e;
  if ((e = hipMemcpyAsync(hm, c->gs->meta.p, kMetaWords * 4, hipMemcpyDeviceToHost, c->ctx->stream)) ||
      (e = stream_wait(c->ctx->stream)))
    return c->ctx->hip_fail(e, "gset meta");
  return CE_OK;
}

// rehash one of the tables into new_cap slots (its count is rebuilt by the claims)
int rehash(ce_core* c, bool is_batch, uint32_t new_cap) {
  GsState* g = c->gs;
  hipStream_t s = c->ctx->stream;
  DevBuf nb;
  hipError_t e;
  uint32_t* meta = g->meta.as<uint32_t>();
  if ((e = nb.reserve((size_t)new_cap * 8)) || (e = hipMemsetAsync(nb.p, 0, (size_t)new_cap * 8, s)) ||
      (e = hipMemsetAsync(meta + 8, 0, 16, s)))
    return c->ctx->hip_fail(e, "gset grow");
  const GsTable src = is_batch ? batch(g) : committed(g);
  const GsTable dst{nb.as<unsigned long long>(), new_cap - 1, new_cap / 2, meta + 8};
  if ((e = launch_gs_move(s, src, dst)) ||
      (e = hipMemcpyAsync(src.meta, meta + 8, 16, hipMemcpyDeviceToDevice, s)) || (e = stream_wait(s)))
    return c->ctx->hip_fail(e, "gset grow");
  if (is_batch) {
    g->bslots = std::move(nb);
    g->bcap = new_cap;
  } else {
    g->slots = std::move(nb);
    g->cap = new_cap;
  }
  c->path_counts[is_batch ? "gset_batch_grows" : "gset_grows"]++;
  return CE_OK;
}

// room in the committed table for `extra` more claims (count: its claims now)
int ensure_committed(ce_core* c, uint64_t count, uint64_t extra) {
  GsState* g = c->gs;
  if (count + extra <= g->cap / 2) return CE_OK;
  if (count + extra > (1ull << 30)) return c->ctx->fail(CE_ERR_INVALID_ARG, "set too large for the table");
  return rehash(c, false, pow2_at_least(2 * (count + extra)));
}

int clear_batch(ce_core* c) {
  GsState* g = c->gs;
  hipError_t e;
  if ((e = hipMemsetAsync(g->bslots.p, 0, (size_t)g->bcap * 8, c->ctx->stream)) ||
      (e = hipMemsetAsync(g->meta.as<uint32_t>() + 4, 0, 16, c->ctx->stream)))
    return c->ctx->hip_fail(e, "gset batch clear");
  g->batch_dirty = false;
  return CE_OK;
}

// decode the files of `only` (null: all; large_only: those of more than one page) from their
// plaintext in HBM into the batch table, growing it until the pass fits
int decode_pass(ce_core* c, uint32_t n, const uint8_t* only, bool large_only = false) {
  ce_ctx* ctx = c->ctx;
  GsState* g = c->gs;
  hipError_t e;
  for (int round = 0;; round++) {
    GsDecodeArgs a{};
    a.pt = ctx->out.as<uint8_t>();
    a.params = ctx->params.as<FileParams>();
    a.status = ctx->status.as<int32_t>();
    a.n = n;
    a.supported = c->d_supported.as<uint8_t>();
    a.n_supported = (uint32_t)c->supported.size();
    a.apply = ctx->apply.as<uint8_t>();
    a.only = only;
    a.large_only = large_only ? 1 : 0;
    a.committed = committed(g);
    a.batch = batch(g);
    a.paths = g->meta.as<uint32_t>() + 12;
    if ((e = hipMemsetAsync(a.paths, 0, 12, ctx->stream))) return ctx->hip_fail(e, "gset decode");
    const int t = ctx->tbegin("decode_gset");
    if ((e = launch_decode_gset(ctx->stream, a, grid_waves_for(n)))) return ctx->hip_fail(e, "gset decode");
    ctx->tend(t);
    g->batch_dirty = true;
    uint32_t hm[kMetaWords];
    int rc = read_meta(c, hm);
    if (rc) return rc;
    if (!hm[4 + kGsOverflow]) {
      c->path_counts["gset_uniform_files"] += hm[12];
      c->path_counts["gset_general_files"] += hm[13];
      return CE_OK;
    }
    if (round > 32 || g->bcap >= (1u << 31)) return ctx->fail(CE_ERR_DEVICE, "batch table did not converge");
    if ((e = hipMemsetAsync(g->meta.as<uint32_t>() + 4 + kGsOverflow, 0, 4, ctx->stream)))
      return ctx->hip_fail(e, "gset decode");
    if ((rc = rehash(c, true, g->bcap * 2))) return rc;
  }
}

int download_status(ce_core* c, uint32_t n, std::vector<int32_t>* st) {
  st->resize(n);
  hipError_t e;
  if ((e = hipMemcpyAsync(st->data(), c->ctx->status.p, n * 4ull, hipMemcpyDeviceToHost, c->ctx->stream)) ||
      (e = stream_wait(c->ctx->stream)))
    return c->ctx->hip_fail(e, "status");
  return CE_OK;
}

// the batch table's members into the committed table
int commit_batch(ce_core* c) {
  GsState* g = c->gs;
  uint32_t hm[kMetaWords];
  int rc = read_meta(c, hm);
  if (rc) return rc;
  if (hm[4 + kGsCount] == 0 && hm[4 + kGsZero] == 0) return clear_batch(c);
  if ((rc = ensure_committed(c, hm[kGsCount], hm[4 + kGsCount]))) return rc;
  hipError_t e;
  const int t = c->ctx->tbegin("gset_commit");
  if ((e = launch_gs_move(c->ctx->stream, batch(g), committed(g)))) return c->ctx->hip_fail(e, "gset commit");
  c->ctx->tend(t);
  return clear_batch(c);
}

bool read_members(Rd& r, std::vector<uint64_t>* out) {
  uint64_t cnt;
  if (!rd_array_hdr(r, &cnt) || cnt > r.n - r.i) return false;  // each element takes >= 1 byte
  out->reserve(out->size() + cnt);
  for (uint64_t k = 0; k < cnt; k++) {
    uint64_t v;
    if (!rd_u64(r, &v)) return false;
    out->push_back(v);
  }
  return true;
}

}  // namespace

bool parse_gset_ops(const uint8_t* p, size_t n, std::vector<uint64_t>* out) {
  Rd r{p, n, 0};
  return read_members(r, out);
}

bool read_gset_state(Rd& r, std::vector<uint64_t>* out) {
  return read_struct(r, {"value"}, [&](int, Rd& q) { return read_members(q, out); });
}

void write_gset_state(Wr* w, const std::vector<uint64_t>& sorted_members) {
  w->map(1);
  w->str("value");
  w->arr(sorted_members.size());
  for (uint64_t v : sorted_members) w->uint(v);
}

int gs_init(ce_core* c) {
  GsState* g = c->gs = new GsState();
  uint32_t cap = 1u << 16;
  if (const char* e = getenv("CE_GSET_CAP")) cap = pow2_at_least((uint64_t)std::max(1l, atol(e)));
  g->cap = g->bcap = cap;
  hipError_t e;
  hipStream_t s = c->ctx->stream;
  if ((e = g->slots.reserve((size_t)cap * 8)) || (e = g->bslots.reserve((size_t)cap * 8)) ||
      (e = g->meta.reserve(kMetaWords * 4)) || (e = hipMemsetAsync(g->slots.p, 0, (size_t)cap * 8, s)) ||
      (e = hipMemsetAsync(g->bslots.p, 0, (size_t)cap * 8, s)) ||
      (e = hipMemsetAsync(g->meta.p, 0, kMetaWords * 4, s)) || (e = stream_wait(s)))
    return c->ctx->hip_fail(e, "gset init");
  return CE_OK;
}

int gs_reset(ce_core* c) {
  GsState* g = c->gs;
  hipError_t e;
  if ((e = hipMemsetAsync(g->slots.p, 0, (size_t)g->cap * 8, c->ctx->stream)) ||
      (e = hipMemsetAsync(g->meta.p, 0, kMetaWords * 4, c->ctx->stream)))
    return c->ctx->hip_fail(e, "gset reset");
  c->pending = false;  // a pending sharded batch goes with the set
  return clear_batch(c);
}

int gs_settle(ce_core* c) {
  hipError_t e = stream_wait(c->ctx->stream);
  return e ? c->ctx->hip_fail(e, "settle") : CE_OK;
}

int gs_insert_members(ce_core* c, const std::vector<uint64_t>& members) {
  if (members.empty()) return CE_OK;
  if (members.size() > (1u << 30)) return c->ctx->fail(CE_ERR_INVALID_ARG, "too many members");
  GsState* g = c->gs;
  uint32_t hm[kMetaWords];
  int rc = read_meta(c, hm);
  if (rc || (rc = ensure_committed(c, hm[kGsCount], members.size()))) return rc;
  hipError_t e;
  hipStream_t s = c->ctx->stream;
  if ((e = g->col.reserve(members.size() * 8 + 64)) ||
      (e = hipMemcpyAsync(g->col.p, members.data(), members.size() * 8, hipMemcpyHostToDevice, s)) ||
      (e = launch_gs_insert(s, committed(g), g->col.as<unsigned long long>(), (uint32_t)members.size())) ||
      (e = stream_wait(s)))  // (the upload reads the caller's vector)
    return c->ctx->hip_fail(e, "gset insert");
  return CE_OK;
}

namespace {

// The head of a StateWrapper exactly as the writer leaves it: 82 b0"next_op_versions" <clock>
// a5"state" 81 a5"value" <array header>.  0: found, *nov / *count / *body (the first element's
// offset) set; 1: another shape (the host parser's); 2: the prefix ended inside the head.
int parse_state_head(const uint8_t* p, uint64_t n, bool whole, Dots* nov, uint64_t* count, uint64_t* body) {
  Rd r{p, n, 0};
  const int cut = whole ? 1 : 2;
  auto lit = [&](const char* s, uint64_t l) -> int {
    const uint64_t have = std::min<uint64_t>(l, r.n - r.i);
    if (std::memcmp(r.p + r.i, s, have) != 0) return 1;
    if (have < l) return cut;
    r.i += l;
    return 0;
  };
  if (int x = lit("\x82\xb0next_op_versions", 18)) return x;
  nov->clear();
  if (!read_vclock(r, nov)) return cut;
  if (int x = lit("\xa5state\x81\xa5value", 13)) return x;
  if (r.i < r.n && !is_array_marker(r.p[r.i])) return 1;
  if (!rd_array_hdr(r, count)) return cut;
  *body = r.i;
  return 0;
}

bool read_gset_wrapper(const uint8_t* p, size_t n, Dots* nov, std::vector<uint64_t>* members) {
  Rd r{p, n, 0};
  return read_struct(r, {"next_op_versions", "state"},
                     [&](int f, Rd& q) { return f == 0 ? read_vclock(q, nov) : read_gset_state(q, members); });
}

constexpr uint32_t kRunWidth[5] = {1, 2, 3, 5, 9};

}  // namespace

// files i = StateWrapper plaintexts at base + off[i], len[i] bytes, st[i] = status so far.  The
// heads are parsed on the host from a prefix; a body whose element widths never decrease is proven
// on the device (k_gs_state_runs) and inserted from HBM (k_gs_state_insert); every other file is
// downloaded whole for the host parser, whose verdict it keeps.  Nothing is inserted before every
// file has its status.  Host waits: the heads, the run table, the inserts' end (which reads the
// table's counts: a launch that met the load bound costs a rehash and a second pass).
int gs_merge_states_device(ce_core* c, const uint8_t* base, const std::vector<uint64_t>& off,
                           const std::vector<uint64_t>& len, int32_t* st, int32_t* status_out) {
  ce_ctx* ctx = c->ctx;
  GsState* g = c->gs;
  hipStream_t s = ctx->stream;
  const size_t n = off.size();
  hipError_t e;
  int rc;
  std::vector<Dots> novs(n);
  std::vector<uint64_t> host_members;
  std::vector<uint8_t> whole;
  uint64_t n_dev = 0, n_host = 0;  // (counted when the call has taken its files)
  auto host_parse = [&](size_t i) -> int {  // the whole plaintext through the host parser
    n_host++;
    whole.resize(len[i]);
    if (len[i] && ((e = hipMemcpyAsync(whole.data(), base + off[i], len[i], hipMemcpyDeviceToHost, s)) ||
                   (e = stream_wait(s))))
      return ctx->hip_fail(e, "state download");
    novs[i].clear();
    if (!read_gset_wrapper(whole.data(), len[i], &novs[i], &host_members)) st[i] = CE_ERR_DECODE;
    return CE_OK;
  };
  // 1) the heads: one prefix per file into pinned memory, one wait
  const uint64_t hint = g->head_hint;
  std::vector<uint64_t> poff(n + 1, 0);
  for (size_t i = 0; i < n; i++) poff[i + 1] = poff[i] + (st[i] == CE_OK ? std::min<uint64_t>(len[i], hint) : 0);
  const uint64_t files_at = (poff[n] + 63) & ~63ull;
  const uint64_t runs_at = files_at + sizeof(GsStateFile) * n;
  const uint64_t table_bytes = 4ull * kGsStateRunWords * n;
  const uint64_t meta_at = runs_at + table_bytes;  // the committed table's counts before the inserts
  if ((e = g->h_rd.reserve(meta_at + 4ull * kMetaWords + 64)) ||
      (e = g->rd.reserve(sizeof(GsStateFile) * n + table_bytes + 64)))
    return ctx->hip_fail(e, "state reader");
  uint8_t* hb = g->h_rd.as<uint8_t>();
  for (size_t i = 0; i < n; i++)
    if (poff[i + 1] > poff[i] &&
        (e = hipMemcpyAsync(hb + poff[i], base + off[i], poff[i + 1] - poff[i], hipMemcpyDeviceToHost, s)))
      return ctx->hip_fail(e, "state head");
  if ((e = stream_wait(s))) return ctx->hip_fail(e, "state head");
  GsStateFile* hf = reinterpret_cast<GsStateFile*>(hb + files_at);
  std::vector<size_t> dev;  // the files the device reads, in descriptor order
  uint64_t head_max = 0;
  uint32_t max_count = 0;
  std::vector<uint8_t> pre;
  for (size_t i = 0; i < n; i++) {
    if (st[i] != CE_OK) continue;
    uint64_t want = poff[i + 1] - poff[i], count = 0, body = 0;
    int pr = parse_state_head(hb + poff[i], want, want == len[i], &novs[i], &count, &body);
    if (pr == 2) {  // a longer head: once more with a larger prefix
      want = std::min<uint64_t>(len[i], want * 16);
      pre.resize(want);
      if ((e = hipMemcpyAsync(pre.data(), base + off[i], want, hipMemcpyDeviceToHost, s)) || (e = stream_wait(s)))
        return ctx->hip_fail(e, "state head");
      pr = parse_state_head(pre.data(), want, want == len[i], &novs[i], &count, &body);
    }
    const uint64_t blen = len[i] - body;
    // (32-bit element offsets: 9 count < 2^32; a count above the bytes left is the host's to refuse)
    if (pr != 0 || blen > 0xffffffffull || 9 * count >= (1ull << 32)) {
      if ((rc = host_parse(i))) return rc;
      continue;
    }
    head_max = std::max(head_max, body);
    hf[dev.size()] = GsStateFile{off[i] + body, (uint32_t)blen, (uint32_t)count, 0, 0};
    max_count = std::max(max_count, (uint32_t)count);
    dev.push_back(i);
  }
  if (head_max) {
    uint64_t h = 1u << 14;
    while (h < head_max + head_max / 4 + 64 && h < (1u << 18)) h <<= 1;
    g->head_hint = h;
  }
  // 2) the runs: five phases over every device file, back to back; the run table comes back in
  //    one download
  const uint32_t nd = (uint32_t)dev.size();
  GsStateFile* d_files = g->rd.as<GsStateFile>();
  uint32_t* d_runs = reinterpret_cast<uint32_t*>(g->rd.as<uint8_t>() + sizeof(GsStateFile) * n);
  const uint32_t* hr = reinterpret_cast<const uint32_t*>(hb + runs_at);
  if (nd) {
    if ((e = hipMemcpyAsync(d_files, hf, sizeof(GsStateFile) * nd, hipMemcpyHostToDevice, s)) ||
        (e = hipMemsetAsync(d_runs, 0xff, 4ull * kGsStateRunWords * nd, s)))
      return ctx->hip_fail(e, "state reader");
    const int t = ctx->tbegin("gset_state_runs");
    if ((e = launch_gs_state_runs(s, base, d_files, nd, max_count, d_runs))) return ctx->hip_fail(e, "state reader");
    ctx->tend(t);
    if ((e = hipMemcpyAsync(hb + runs_at, d_runs, 4ull * kGsStateRunWords * nd, hipMemcpyDeviceToHost, s)) ||
        (e = hipMemcpyAsync(hb + meta_at, g->meta.p, 4ull * kMetaWords, hipMemcpyDeviceToHost, s)) ||
        (e = stream_wait(s)))
      return ctx->hip_fail(e, "state reader");
  }
  // a file whose runs sum to its count is proven, element by element; any other is the host's
  uint64_t dev_members = 0, max_proven = 0;
  for (uint32_t k = 0; k < nd; k++) {
    const uint32_t* R = hr + kGsStateRunWords * k;
    uint64_t sum = 0, end = 0;
    for (int r = 0; r < 5; r++) {
      sum += R[r];
      end += (uint64_t)R[r] * kRunWidth[r];
    }
    if (sum == hf[k].count && end <= hf[k].blen && dev_members + sum <= (1ull << 30)) {
      dev_members += sum;
      max_proven = std::max(max_proven, sum);
      n_dev++;
      continue;
    }
    hf[k].count = 0;  // (skipped by the insert)
    if ((rc = host_parse(dev[k]))) return rc;
  }
  // 3) every file has its status: all or nothing (lib.rs:425-466)
  if (status_out) std::memcpy(status_out, st, n * 4ull);
  for (size_t i = 0; i < n; i++)
    if (st[i] != CE_OK) return ctx->fail(st[i], st[i] == CE_ERR_DECODE ? "not a StateWrapper" : "state file rejected");
  // 4) the members: the proven files in launches of kGsStateMaxFiles, then the host-parsed ones
  // (a table that cannot hold even the largest file's members is grown ahead: a new replica's
  // first compaction would otherwise pay a pass that is certain to meet the load bound)
  if (dev_members && max_proven > g->cap / 2 &&
      (rc = ensure_committed(c, reinterpret_cast<const uint32_t*>(hb + meta_at)[kGsCount], dev_members)))
    return rc;
  for (int pass = 0; dev_members; pass++) {
    for (uint32_t k0 = 0; k0 < nd; k0 += kGsStateMaxFiles) {
      const uint32_t k = std::min(kGsStateMaxFiles, nd - k0);
      uint32_t total = 0;
      for (uint32_t j = 0; j < k; j++) {
        hf[k0 + j].pre = total;
        total += hf[k0 + j].count;
      }
      if (total == 0) continue;
      if (pass == 0 &&
          (e = hipMemcpyAsync(d_files + k0, hf + k0, sizeof(GsStateFile) * k, hipMemcpyHostToDevice, s)))
        return ctx->hip_fail(e, "state insert");
      const int t = ctx->tbegin("gset_state_insert");
      if ((e = launch_gs_state_insert(s, committed(g), base, d_files + k0, k, total, d_runs + kGsStateRunWords * k0)))
        return ctx->hip_fail(e, "state insert");
      ctx->tend(t);
    }
    // The table is not grown ahead for members it may already hold (a compaction mostly repeats
    // the one before it).  The wait that ends the call reads its counts back: a launch that met
    // the load bound is run once more (inserts are idempotent) after one growth, to room for
    // the members the table held before the call (read with the run table) and every member of
    // the call.
    uint32_t now[kMetaWords];
    if ((rc = read_meta(c, now))) return rc;
    if (!now[kGsOverflow]) break;
    if (pass) return ctx->fail(CE_ERR_DEVICE, "committed table did not take the state files");
    const uint32_t before = reinterpret_cast<const uint32_t*>(hb + meta_at)[kGsCount];
    if ((e = hipMemsetAsync(g->meta.as<uint32_t>() + kGsOverflow, 0, 4, s))) return ctx->hip_fail(e, "gset grow");
    if ((rc = ensure_committed(c, before, dev_members))) return rc;
  }
  if ((rc = gs_insert_members(c, host_members))) return rc;
  // state.merge done; next_op_versions.merge(sw.next_op_versions) (lib.rs:461-463)
  for (size_t i = 0; i < n; i++)
    for (auto& d : novs[i]) {
      uint32_t slot;
      if ((rc = insert_actor(c, d.first, &slot))) return rc;
      c->nov[slot] = std::max(c->nov[slot], d.second);
    }
  if ((rc = table_upload(c))) return rc;
  // (the plaintexts may be the caller's buffer: the inserts have been waited for above)
  c->path_counts["gset_states_device_read"] += n_dev;
  c->path_counts["gset_states_host_read"] += n_host;
  return CE_OK;
}

// the set in BTreeSet order in g->sorted (device): the live slots collected, then the radix sort
// (ce_ser_sort.hip's generic u64 key mode); *n_out = the member count
static int collect_sorted(ce_core* c, uint32_t* n_members) {
  GsState* g = c->gs;
  hipStream_t s = c->ctx->stream;
  uint32_t hm[kMetaWords];
  int rc = read_meta(c, hm);
  if (rc) return rc;
  const uint32_t n = *n_members = hm[kGsCount] + (hm[kGsZero] ? 1u : 0u);
  if (n == 0) return CE_OK;
  hipError_t e;
  uint32_t* n_out = g->meta.as<uint32_t>() + 15;
  size_t tb = 0;
  if ((e = g->col.reserve((size_t)n * 8 + 64)) || (e = g->sorted.reserve((size_t)n * 8 + 64)) ||
      (e = g->vals.reserve((size_t)n * 8 + 64)) ||
      (e = sort_pairs_u64(nullptr, tb, nullptr, nullptr, nullptr, nullptr, n, 64, s)) ||
      (e = g->sort_tmp.reserve(tb + 256)))
    return c->ctx->hip_fail(e, "gset collect");
  tb = g->sort_tmp.cap;
  uint32_t* vin = g->vals.as<uint32_t>();
  const int t = c->ctx->tbegin("gset_sort");  // (the collect and the radix sort's passes)
  if ((e = hipMemsetAsync(n_out, 0, 4, s)) ||
      (e = launch_gs_collect(s, committed(g), g->col.as<unsigned long long>(), n_out)) ||
      (e = sort_pairs_u64(g->sort_tmp.p, tb, g->col.as<unsigned long long>(), g->sorted.as<unsigned long long>(),
                          vin, vin + n, n, 64, s)))
    return c->ctx->hip_fail(e, "gset collect");
  c->ctx->tend(t);
  return CE_OK;
}

int gs_members_sorted(ce_core* c, std::vector<uint64_t>* out) {
  uint32_t n = 0;
  int rc = collect_sorted(c, &n);
  if (rc) return rc;
  out->resize(n);
  hipError_t e;
  if (n && ((e = hipMemcpyAsync(out->data(), c->gs->sorted.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->ctx->stream)) ||
            (e = stream_wait(c->ctx->stream))))
    return c->ctx->hip_fail(e, "gset collect");
  return CE_OK;
}

// ---- with_state reads (lib.rs:325-330): the committed table only; a batch left pending by the
// sharded ingest lives in the batch table and is no part of any answer ----

// GSet::contains over a query column in HBM; complete on return
int gs_contains_device(ce_core* c, const uint64_t* d_members, uint64_t n, uint8_t* d_out) {
  if (n == 0) return CE_OK;
  ce_ctx* ctx = c->ctx;
  hipError_t e;
  const int t = ctx->tbegin("gs_contains");
  if ((e = launch_gs_contains(ctx->stream, committed(c->gs), reinterpret_cast<const unsigned long long*>(d_members), n,
                              d_out, test_grid_cap())))
    return ctx->hip_fail(e, "gset contains");
  ctx->tend(t);
  if ((e = stream_wait(ctx->stream))) return ctx->hip_fail(e, "gset contains");
  return CE_OK;
}

// read().val.len(): the claimed slots and the out-of-band member 0
int gs_set_len(ce_core* c, uint64_t* n) {
  uint32_t hm[kMetaWords];
  int rc = read_meta(c, hm);
  if (rc) return rc;
  *n = (uint64_t)hm[kGsCount] + (hm[kGsZero] ? 1u : 0u);
  return CE_OK;
}

// read().val ascending into d_dst: the serializer's collect and sort, then one device copy
int gs_members_device(ce_core* c, uint64_t* d_dst, uint64_t cap, uint64_t* n) {
  int rc = gs_set_len(c, n);
  if (rc || *n == 0 || cap < *n) return rc;
  uint32_t got = 0;
  if ((rc = collect_sorted(c, &got))) return rc;
  hipError_t e;
  if ((e = hipMemcpyAsync(d_dst, c->gs->sorted.p, (size_t)got * 8, hipMemcpyDeviceToDevice, c->ctx->stream)) ||
      (e = stream_wait(c->ctx->stream)))
    return c->ctx->hip_fail(e, "gset members");
  return CE_OK;
}

namespace {

// The device writer.  head: the clear text up to and including a5"state" (the host's part: the
// optional data version and next_op_versions).  Into ctx->blob: head, 81 a5"value", the array
// header and the members ascending, each in its smallest form; at A = *args_at (past the clear
// text's bound) the seal's small arguments [offs(2) | out_offs(1) | nonce (24 B) | outer version
// (16 B)], offs[1] = the clear length, written by the writer's last thread.  Nothing is waited for.
int write_device(ce_core* c, std::vector<uint8_t> head, const uint8_t* nonce, const uint8_t* outer,
                 uint64_t* args_at, uint64_t* bound) {
  ce_ctx* ctx = c->ctx;
  GsState* g = c->gs;
  hipStream_t s = ctx->stream;
  uint32_t n = 0;
  int rc = collect_sorted(c, &n);
  if (rc) return rc;
  if (9ull * n >= (1ull << 32)) return ctx->fail(CE_ERR_INVALID_ARG, "set too large for 32-bit element offsets");
  Wr w;
  w.b.swap(head);
  w.map(1);
  w.str("value");
  w.arr(n);
  const uint64_t head_len = w.b.size();
  const uint64_t U = *bound = head_len + 9ull * n;
  const uint64_t A = *args_at = (U + 255) & ~255ull;
  hipError_t e;
  if ((e = ctx->blob.reserve(A + 128)) || (e = ctx->h_stage.reserve(head_len + 64 + 256)) ||
      (e = g->vals.reserve((size_t)n * 8 + 64)))
    return ctx->hip_fail(e, "gset writer");
  uint8_t* hs = ctx->h_stage.as<uint8_t>();
  uint8_t* db = ctx->blob.as<uint8_t>();
  const uint64_t args[3] = {0, head_len, 0};  // offs[1]: an empty set's clear length
  std::memcpy(hs, w.b.data(), head_len);
  uint8_t* ha = hs + ((head_len + 7) & ~7ull);
  std::memset(ha, 0, 64);
  std::memcpy(ha, args, 24);
  if (nonce) std::memcpy(ha + 24, nonce, 24);
  if (outer) std::memcpy(ha + 48, outer, 16);
  if ((e = hipMemcpyAsync(db, hs, head_len, hipMemcpyHostToDevice, s)) ||
      (e = hipMemcpyAsync(db + A, ha, 64, hipMemcpyHostToDevice, s)))
    return ctx->hip_fail(e, "gset writer");
  c->path_counts["gset_device_writes"]++;
  if (n == 0) return CE_OK;  // (the head is the whole state)
  const unsigned long long* sorted = g->sorted.as<unsigned long long>();
  uint32_t* wid = g->vals.as<uint32_t>();
  uint32_t* off = wid + n;
  size_t tb = 0;
  if ((e = ds_excl_sum_u32(nullptr, tb, wid, off, n, s)) || (e = g->scan_tmp.reserve(tb + 256)))
    return ctx->hip_fail(e, "gset writer");
  tb = g->scan_tmp.cap;
  const int t = ctx->tbegin("gset_write");
  if ((e = launch_gs_widths(s, sorted, n, wid)) || (e = ds_excl_sum_u32(g->scan_tmp.p, tb, wid, off, n, s)) ||
      (e = launch_gs_write(s, sorted, off, n, db + head_len, reinterpret_cast<unsigned long long*>(db + A + 8),
                           head_len)))
    return ctx->hip_fail(e, "gset writer");
  ctx->tend(t);
  return CE_OK;
}

}  // namespace

int gs_serialize_device(ce_core* c, std::vector<uint8_t> head, std::vector<uint8_t>* out) {
  ce_ctx* ctx = c->ctx;
  uint64_t A = 0, U = 0, clear_len = 0;
  int rc = write_device(c, std::move(head), nullptr, nullptr, &A, &U);
  if (rc) return rc;
  const uint8_t* db = ctx->blob.as<uint8_t>();
  hipError_t e;
  if ((e = hipMemcpyAsync(&clear_len, db + A + 8, 8, hipMemcpyDeviceToHost, ctx->stream)) ||
      (e = stream_wait(ctx->stream)))
    return ctx->hip_fail(e, "gset state bytes");
  if (clear_len > U) return ctx->fail(CE_ERR_DEVICE, "serialized state past its bound");
  out->resize(clear_len);
  if (clear_len && ((e = hipMemcpyAsync(out->data(), db, clear_len, hipMemcpyDeviceToHost, ctx->stream)) ||
                    (e = stream_wait(ctx->stream))))
    return ctx->hip_fail(e, "gset state bytes");
  return CE_OK;
}

// ce_core_state_bytes into device memory: the writer's clear text stays in HBM, only its length
// comes to the host
int gs_state_bytes_device(ce_core* c, std::vector<uint8_t> head, uint8_t* d_dst, uint64_t cap, uint64_t* len) {
  ce_ctx* ctx = c->ctx;
  uint64_t A = 0, U = 0, clear_len = 0;
  int rc;
  {
    HostPhase hp("gset bytes: write");
    if ((rc = write_device(c, std::move(head), nullptr, nullptr, &A, &U))) return rc;
  }
  const uint8_t* db = ctx->blob.as<uint8_t>();
  hipError_t e;
  {
    HostPhase hp("gset bytes: length");
    if ((e = hipMemcpyAsync(&clear_len, db + A + 8, 8, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = stream_wait(ctx->stream)))
      return ctx->hip_fail(e, "gset state bytes");
  }
  if (clear_len > U) return ctx->fail(CE_ERR_DEVICE, "serialized state past its bound");
  *len = clear_len;
  if (clear_len > cap) return ctx->fail(CE_ERR_INVALID_ARG, "device buffer too small for the state");
  // complete on return: the caller's collective may run on another stream
  HostPhase hp("gset bytes: copy");
  if (clear_len && ((e = hipMemcpyAsync(d_dst, db, clear_len, hipMemcpyDeviceToDevice, ctx->stream)) ||
                    (e = stream_wait(ctx->stream))))
    return ctx->hip_fail(e, "gset state bytes");
  c->path_counts["gset_state_bytes_device"]++;
  return CE_OK;
}

int gs_compact_device(ce_core* c, std::vector<uint8_t> head, const uint8_t* outer, const uint8_t* nonce,
                      const KeyRef& key, std::vector<uint8_t>* file) {
  ce_ctx* ctx = c->ctx;
  if (int32_t ks = key_status(key)) return ctx->fail(ks, "key rejected");
  uint8_t nb[24];
  if (nonce) std::memcpy(nb, nonce, 24);
  else os_random(nb, 24);
  uint64_t A = 0, U = 0, clear_len = 0;
  int rc = write_device(c, std::move(head), nb, outer, &A, &U);
  if (rc) return rc;
  hipError_t e;
  if ((e = ctx->out.reserve(16 + sealed_len(U) + 64))) return ctx->hip_fail(e, "gset compact");
  uint8_t* db = ctx->blob.as<uint8_t>();
  if ((rc = device_seal(ctx, db, reinterpret_cast<const uint64_t*>(db + A), 1, U, db + A + 48, db + A + 24,
                        ctx->out.as<uint8_t>(), reinterpret_cast<const uint64_t*>(db + A + 16), key)))
    return rc;
  if ((e = hipMemcpyAsync(&clear_len, db + A + 8, 8, hipMemcpyDeviceToHost, ctx->stream)) ||
      (e = stream_wait(ctx->stream)))
    return ctx->hip_fail(e, "gset compact");
  if (clear_len > U) return ctx->fail(CE_ERR_DEVICE, "serialized state past its bound");
  file->resize(16 + sealed_len(clear_len));
  if ((e = hipMemcpyAsync(file->data(), ctx->out.p, file->size(), hipMemcpyDeviceToHost, ctx->stream)) ||
      (e = stream_wait(ctx->stream)))
    return ctx->hip_fail(e, "gset compact");
  return CE_OK;
}

// ---- the op-file writer: Core::apply_ops (lib.rs:666-722) over a member column in HBM ----

namespace {

// a column of n members at per_file (0: kGsFileMembers) members a file: the files, the most bytes
// they take sealed (every member 9 bytes wide), and the clear texts' bound 19 F + 9 n; false:
// per_file out of range, or more files than a u32 counts
bool apply_bound(uint64_t n, uint32_t* per_file, uint32_t* files, uint64_t* bytes, uint64_t* clear_bound) {
  if (*per_file == 0) *per_file = kGsFileMembers;
  if (*per_file > kGsFileMembers) return false;
  const uint64_t pf = *per_file, full = n / pf, rem = n % pf, F = full + (rem ? 1 : 0);
  if (F > 0xffffffffull) return false;
  *files = (uint32_t)F;
  *bytes = full * (16 + sealed_len(16 + arr_hdr_len((uint32_t)pf) + 9 * pf)) +
           (rem ? 16 + sealed_len(16 + arr_hdr_len((uint32_t)rem) + 9 * rem) : 0);
  *clear_bound = 19 * F + 9 * n;
  return true;
}

// what both forms refuse before anything is touched; *per_file normalised, *max_bytes the bound
int apply_check(ce_core* c, uint64_t n, uint32_t* per_file, uint32_t flags, uint32_t* max_files, uint64_t* max_bytes) {
  ce_ctx* ctx = c->ctx;
  if (c->kind != CE_STATE_GSET) return ctx->fail(CE_ERR_INVALID_ARG, "gset apply: not a GSet core");
  uint64_t clear_bound = 0;
  if (!apply_bound(n, per_file, max_files, max_bytes, &clear_bound))
    return ctx->fail(CE_ERR_INVALID_ARG, "gset apply: per_file is 1..453 (0: 453)");
  if (flags & ~(uint32_t)CE_GSET_APPLY_NEW_ONLY) return ctx->fail(CE_ERR_INVALID_ARG, "gset apply: unknown flags");
  if (clear_bound >= (1ull << 32)) return ctx->fail(CE_ERR_INVALID_ARG, "gset apply: column too large for 32-bit offsets");
  if (!c->has_key) return ctx->fail(CE_ERR_NO_KEY, "no latest key");
  return CE_OK;
}

// CE_GSET_APPLY_NEW_ONLY: the column's distinct members the committed table does not hold,
// ascending, into g->col; *m = how many (the one word the host reads)
int filter_new(ce_core* c, const uint64_t* d_members, uint32_t n, uint32_t* m) {
  ce_ctx* ctx = c->ctx;
  GsState* g = c->gs;
  hipStream_t s = ctx->stream;
  hipError_t e;
  size_t sb = 0, cb = 0;
  if ((e = g->sorted.reserve((size_t)n * 8 + 64)) || (e = g->col.reserve((size_t)n * 8 + 64)) ||
      (e = g->vals.reserve((size_t)n * 8 + 64)) || (e = g->filt.reserve(((size_t)n + 1) * 8 + 64)) ||
      (e = sort_pairs_u64(nullptr, sb, nullptr, nullptr, nullptr, nullptr, n, 64, s)) ||
      (e = g->sort_tmp.reserve(sb + 256)) || (e = ds_excl_sum_u32(nullptr, cb, nullptr, nullptr, n + 1, s)) ||
      (e = g->scan_tmp.reserve(cb + 256)))
    return ctx->hip_fail(e, "gset apply filter");
  sb = g->sort_tmp.cap;
  cb = g->scan_tmp.cap;
  unsigned long long* sorted = g->sorted.as<unsigned long long>();
  uint32_t* vin = g->vals.as<uint32_t>();  // (the sort carries values; nobody reads them)
  uint32_t* keep = g->filt.as<uint32_t>();
  uint32_t* pos = keep + n + 1;
  const int t = ctx->tbegin("gset_apply_filter");
  if ((e = sort_pairs_u64(g->sort_tmp.p, sb, reinterpret_cast<const unsigned long long*>(d_members), sorted, vin,
                          vin + n, n, 64, s)) ||
      (e = launch_gs_new_mark(s, committed(g), sorted, n, keep)) ||
      (e = ds_excl_sum_u32(g->scan_tmp.p, cb, keep, pos, n + 1, s)) ||
      (e = launch_gs_new_compact(s, sorted, keep, pos, n, g->col.as<unsigned long long>())))
    return ctx->hip_fail(e, "gset apply filter");
  ctx->tend(t);
  if ((e = hipMemcpyAsync(m, pos + n, 4, hipMemcpyDeviceToHost, s)) || (e = stream_wait(s)))
    return ctx->hip_fail(e, "gset apply filter");
  if (*m > n) return ctx->fail(CE_ERR_DEVICE, "gset apply: more survivors than members");
  return CE_OK;
}

}  // namespace

// the arguments have passed apply_check; per_file is normalised and cap >= the bound's bytes
int gs_apply_members_device(ce_core* c, const uint64_t* d_members, uint64_t n_in, uint32_t per_file, uint32_t flags,
                            const uint8_t* nonces, uint8_t* d_files, uint64_t* d_file_offs, uint32_t* n_files,
                            uint64_t* bytes) {
  ce_ctx* ctx = c->ctx;
  GsState* g = c->gs;
  hipStream_t s = ctx->stream;
  hipError_t e;
  int rc;
  const unsigned long long* col = reinterpret_cast<const unsigned long long*>(d_members);
  uint32_t n = (uint32_t)n_in;  // (9 n < 2^32)
  if (n && (flags & CE_GSET_APPLY_NEW_ONLY)) {
    uint32_t m = 0;
    if ((rc = filter_new(c, d_members, n, &m))) return rc;
    c->path_counts["gset_apply_filtered"] += n - m;
    col = g->col.as<unsigned long long>();
    n = m;
  }
  const uint32_t F = (n + per_file - 1) / per_file;
  if (F == 0) return opfile_empty(c, "gset apply", d_file_offs, n_files, bytes);
  // room for every member before anything is sealed: the insert below cannot meet the load bound
  uint32_t hm[kMetaWords];
  if ((rc = read_meta(c, hm)) || (rc = ensure_committed(c, hm[kGsCount], n))) return rc;
  const uint64_t U = 19ull * F + 9ull * n;
  size_t cb = 0;
  if ((e = g->wr.reserve(24ull * (F + 1) + 64)) || (e = ds_excl_sum_u32(nullptr, cb, nullptr, nullptr, F + 1, s)) ||
      (e = g->scan_tmp.reserve(cb + 256)))
    return ctx->hip_fail(e, "gset apply reserve");
  GsFilesArgs a{};
  a.members = col;
  a.n = n;
  a.per_file = per_file;
  a.L.n_files = F;
  unsigned long long* offs = g->wr.as<unsigned long long>();
  opfile_carve(c, offs, reinterpret_cast<uint32_t*>(offs + F + 1), F + 1, d_file_offs, &a.L);
  std::vector<uint8_t> drawn;
  if ((rc = opfile_stage(c, "gset apply", U, nonces, &drawn, &a.L))) return rc;
  int t = ctx->tbegin("gset_apply_sizes");  // (the size pass and its two scans)
  if ((e = launch_gs_file_sizes(s, a)) || (e = opfile_scan(a.L, g->scan_tmp.p, g->scan_tmp.cap, s)))
    return ctx->hip_fail(e, "gset apply sizes");
  ctx->tend(t);
  t = ctx->tbegin("gset_apply_encode");
  if ((e = launch_gs_files_encode(s, a, test_grid_cap()))) return ctx->hip_fail(e, "gset apply encode");
  ctx->tend(t);
  // everything is sealed behind the wait: stored, inserted and bumped from there on
  uint64_t total = 0, v0 = 0;
  if ((rc = opfile_seal(c, "gset apply", a.L, U, d_files, &total)) ||
      (rc = opfile_store(c, "gset apply", a.L, d_files, total, &v0)))
    return rc;
  // state.apply(op) for op in ops (lib.rs:710-712): from the column, or the survivors, in HBM
  t = ctx->tbegin("gset_apply_insert");
  if ((e = launch_gs_insert(s, committed(g), col, n))) return ctx->hip_fail(e, "gset apply insert");
  ctx->tend(t);
  if ((e = stream_wait(s))) return ctx->hip_fail(e, "gset apply insert");  // (the column is the caller's)
  c->path_counts["gset_apply_device_files"] += F;
  c->path_counts["gset_apply_device_members"] += n;
  *n_files = F;
  *bytes = total;
  return opfile_finish(c, v0, F);
}

namespace {

// what the gate leaves for the commit: the writers' slots, next_op_versions after the applied
// files (lib.rs:537-538) and where the fold stopped
struct GsGate {
  std::vector<uint32_t> wslot;
  uint64_t gen0 = 0;
  std::vector<uint64_t> expect;
  uint32_t first_gap = 0xffffffffu;  // host gate: the file at the gap (n: none)
  bool gap = false;                  // window gate: the windows stop at a gap
};

// writers get slots first (the gate is keyed by them); the batch's scratch; a batch table left
// by an earlier ingest (rejected, or pending and never committed) is dropped
int prepare_ingest(ce_core* c, uint32_t n, uint64_t blob_len, const uint8_t* actors, uint32_t m, GsGate* gt) {
  ce_ctx* ctx = c->ctx;
  GsState* g = c->gs;
  hipError_t e;
  int rc;
  gt->wslot.resize(m);
  gt->gen0 = c->table_gen;
  for (uint32_t a = 0; a < m; a++) {
    Uuid u;
    std::memcpy(u.data(), actors + 16ull * a, 16);
    if ((rc = insert_actor(c, u, &gt->wslot[a]))) return rc;
  }
  if (c->table_gen != gt->gen0) refresh_slots(c, actors, m, &gt->wslot);
  if ((rc = table_upload(c)) || (rc = ensure_supported(c))) return rc;
  if ((e = ctx->out.reserve(blob_len + 16ull * n + 128)) || (e = ctx->status.reserve(n * 4ull + 64)) ||
      (e = ctx->apply.reserve(n + 64)) || (e = g->only.reserve(n + 64)))
    return ctx->hip_fail(e, "ingest reserve");
  if (g->batch_dirty && (rc = clear_batch(c))) return rc;
  gt->expect.resize(m);
  for (uint32_t a = 0; a < m; a++) gt->expect[a] = c->nov[gt->wslot[a]];
  return CE_OK;
}

// the version gate (lib.rs:519-538) on the host: it needs no plaintext
int gate_host(ce_core* c, uint32_t n, uint32_t m, const uint32_t* d_fa, const uint64_t* d_fv, GsGate* gt) {
  ce_ctx* ctx = c->ctx;
  hipError_t e;
  std::vector<uint32_t> fa(n);
  std::vector<uint64_t> fv(n);
  std::vector<uint8_t> ap(n);
  if ((e = hipMemcpyAsync(fa.data(), d_fa, n * 4ull, hipMemcpyDeviceToHost, ctx->stream)) ||
      (e = hipMemcpyAsync(fv.data(), d_fv, n * 8ull, hipMemcpyDeviceToHost, ctx->stream)) ||
      (e = stream_wait(ctx->stream)))
    return ctx->hip_fail(e, "gate");
  for (uint32_t i = 0; i < n; i++)
    if (fa[i] >= m) return ctx->fail(CE_ERR_INVALID_ARG, "file_actor out of range");
  gt->first_gap = host_gate(fa.data(), fv.data(), n, &gt->expect, ap.data());
  if ((e = hipMemcpyAsync(ctx->apply.p, ap.data(), n, hipMemcpyHostToDevice, ctx->stream)) ||
      (e = stream_wait(ctx->stream)))
    return ctx->hip_fail(e, "gate");
  return CE_OK;
}

// Every file opened, checked and decoded whatever the gate says, the gated files' members (apply[],
// already on the device) into the batch table.  A failing file: its status is returned, the batch
// table is cleared and the committed set untouched (all-or-nothing, lib.rs:497-514).
int fold_batch(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n, uint64_t blob_len,
               int32_t* status_out) {
  ce_ctx* ctx = c->ctx;
  GsState* g = c->gs;
  hipError_t e;
  int rc;
  // single-page files: opened, checked and decoded in one kernel, the plaintext in LDS
  // (k_open_fold_v3's GS form, lib.rs:501-507), the gated files' members into the batch table;
  // larger files: opened to HBM by the segment pass and decoded whole by k_decode_gset
  uint32_t ec = 0;
  if ((rc = device_open_setup(ctx, d_blob, d_offs, n, blob_len, true, key_of(c), ctx->status.as<int32_t>(), &ec)))
    return rc;
  uint32_t* paths = g->meta.as<uint32_t>() + 12;
  g->h_fused = GsFused{committed(g), batch(g), paths};
  if ((e = g->fused.reserve(sizeof(GsFused))) || (e = hipMemsetAsync(paths, 0, 12, ctx->stream)) ||
      (e = hipMemcpyAsync(g->fused.p, &g->h_fused, sizeof(GsFused), hipMemcpyHostToDevice, ctx->stream)))
    return ctx->hip_fail(e, "gset fused args");
  DecodeArgs da{};
  da.pt = ctx->out.as<uint8_t>();
  da.blob = d_blob;
  da.params = ctx->params.as<FileParams>();
  da.status = ctx->status.as<int32_t>();
  da.n = n;
  da.supported = c->d_supported.as<uint8_t>();
  da.n_supported = (uint32_t)c->supported.size();
  da.apply = ctx->apply.as<uint8_t>();
  da.counters = ctx->counters.as<uint32_t>();
  da.aux = ctx->poly_aux.as<PolyAux>();
  da.gs = g->fused.as<GsFused>();
  ctx->open_log.grid_cap = test_grid_cap();
  ctx->open_log.stamps = test_wave_stamps(ctx);
  ctx->open_log.stamp_waves = 0;  // this ingest's launches, if stamped, are the ones to read
  {
    hipEvent_t t0, t1;
    (void)ctx->tlaunch("open_fold_small", &t0, &t1);
    if ((e = launch_open_fold_gset(ctx->stream, da, ctx->open_log, t0, t1))) return ctx->hip_fail(e, "fused");
  }
  g->batch_dirty = true;
  const SegScratch sc = segscratch(ctx, ec);
  int t = ctx->tbegin("segments_open");
  if ((e = launch_segments(ctx->stream, false, d_blob, ctx->out.as<uint8_t>(), ctx->params.as<FileParams>(), n,
                           ctx->status.as<int32_t>(), sc, grid_waves_for(n + ec), true)))
    return ctx->hip_fail(e, "open segments");
  ctx->tend(t);
  t = ctx->tbegin("finalize_open");
  if ((e = launch_finalize_multi(ctx->stream, false, ctx->out.as<uint8_t>(), ctx->params.as<FileParams>(),
                                 ctx->status.as<int32_t>(), sc, n)))
    return ctx->hip_fail(e, "open finalize");
  ctx->tend(t);
  count_open_launches(c, ctx);
  uint32_t hm[kMetaWords], hc[16];
  if ((e = hipMemcpyAsync(hc, ctx->counters.p, 64, hipMemcpyDeviceToHost, ctx->stream))) return ctx->hip_fail(e, "counters");
  if ((rc = read_meta(c, hm))) return rc;
  std::vector<int32_t> st;
  if (hm[4 + kGsOverflow]) {
    // the batch table filled up inside the fused open: grown, then the batch folded again from
    // plaintext in HBM (inserts are idempotent; every file is opened and checked again)
    if ((e = hipMemsetAsync(g->meta.as<uint32_t>() + 4 + kGsOverflow, 0, 4, ctx->stream))) return ctx->hip_fail(e, "gset grow");
    if ((rc = rehash(c, true, g->bcap * 2)) ||
        (rc = device_open(ctx, d_blob, d_offs, n, blob_len, true, key_of(c), ctx->out.as<uint8_t>(),
                          ctx->status.as<int32_t>(), false, true)))
      return rc;
    count_open_launches(c, ctx);
    c->path_counts["gset_refolds"]++;
    if ((rc = download_status(c, n, &st))) return rc;
    if (std::find(st.begin(), st.end(), kStatusHostParse) != st.end()) {
      if ((rc = resolve_host_parse(c, d_blob, d_offs, n, true))) return rc;
    }
    if ((rc = decode_pass(c, n, nullptr)) || (rc = download_status(c, n, &st))) return rc;
  } else {
    c->path_counts["gset_fused_files"] += hm[14];
    c->path_counts["gset_uniform_files"] += hm[12];
    c->path_counts["gset_general_files"] += hm[13];
    if (hc[9] && (rc = decode_pass(c, n, nullptr, true))) return rc;  // files of more than one page
    if ((rc = download_status(c, n, &st))) return rc;
    if (std::find(st.begin(), st.end(), kStatusHostParse) != st.end()) {
      // envelopes left to the host: opened there, the plaintext patched into HBM, decoded from it
      std::vector<uint8_t> sel(n);
      for (uint32_t i = 0; i < n; i++) sel[i] = st[i] == kStatusHostParse;
      if ((rc = resolve_host_parse(c, d_blob, d_offs, n, true))) return rc;
      if ((e = hipMemcpyAsync(g->only.p, sel.data(), n, hipMemcpyHostToDevice, ctx->stream)) ||
          (e = stream_wait(ctx->stream)))
        return ctx->hip_fail(e, "host parse mask");
      if ((rc = decode_pass(c, n, g->only.as<uint8_t>())) || (rc = download_status(c, n, &st))) return rc;
    }
  }
  // CE_OPEN_MULTI_KEY: files that failed authentication under the latest key, under each other
  // key of the set in id order (the whole batch is opened again; only those files are decoded)
  if ((c->flags & CE_OPEN_MULTI_KEY) && !c->alt_keys.empty()) {
    bool any_auth = false, only_auth = true;
    for (int32_t s : st) {
      any_auth |= s == CE_ERR_AUTH;
      only_auth &= s == CE_OK || s == CE_ERR_AUTH;
    }
    if (any_auth && only_auth) {
      std::vector<int32_t> sk;
      std::vector<uint8_t> sel(n);
      for (const AltKey& ak : c->alt_keys) {
        if (std::find(st.begin(), st.end(), (int32_t)CE_ERR_AUTH) == st.end()) break;
        const KeyRef kr{ak.version, ak.key.data(), ak.key.size()};
        if ((rc = device_open(ctx, d_blob, d_offs, n, blob_len, true, kr, ctx->out.as<uint8_t>(),
                              ctx->status.as<int32_t>(), false)) ||
            (rc = download_status(c, n, &sk)))
          return rc;
        bool opened = false;
        for (uint32_t i = 0; i < n; i++) opened |= (sel[i] = st[i] == CE_ERR_AUTH && sk[i] == CE_OK) != 0;
        if (!opened) continue;
        if ((e = hipMemcpyAsync(g->only.p, sel.data(), n, hipMemcpyHostToDevice, ctx->stream)) ||
            (e = stream_wait(ctx->stream)))
          return ctx->hip_fail(e, "multi-key mask");
        if ((rc = decode_pass(c, n, g->only.as<uint8_t>())) || (rc = download_status(c, n, &sk))) return rc;
        for (uint32_t i = 0; i < n; i++)
          if (sel[i]) st[i] = sk[i];
      }
    }
  }
  if (status_out) std::memcpy(status_out, st.data(), n * 4ull);
  for (uint32_t i = 0; i < n; i++)
    if (st[i] != CE_OK) {  // all-or-nothing: the batch table is dropped, the set untouched
      if ((rc = clear_batch(c))) return rc;
      return st[i];
    }
  return CE_OK;
}

}  // namespace

int gs_ingest_ops(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                  uint64_t blob_len, const uint8_t* actors, uint32_t m, const uint32_t* d_fa,
                  const uint64_t* d_fv, int32_t* status_out) {
  GsGate gt;
  int rc;
  if ((rc = prepare_ingest(c, n, blob_len, actors, m, &gt)) || (rc = gate_host(c, n, m, d_fa, d_fv, &gt)) ||
      (rc = fold_batch(c, d_blob, d_offs, n, blob_len, status_out)))
    return rc;
  // commit, next_op_versions (lib.rs:537-538) and the gap error (lib.rs:527-531)
  if ((rc = commit_batch(c))) return rc;
  if (c->table_gen != gt.gen0) refresh_slots(c, actors, m, &gt.wslot);
  for (uint32_t w = 0; w < m; w++) c->nov[gt.wslot[w]] = std::max(c->nov[gt.wslot[w]], gt.expect[w]);
  if (gt.first_gap < n) {
    if (status_out) status_out[gt.first_gap] = CE_ERR_OP_VERSION;
    return CE_ERR_OP_VERSION;
  }
  return CE_OK;
}

// The sharded ingest (crdtenc shard.ingest_gset_sharded): the same fold with the agreed windows
// as the gate, the batch table left PENDING for ce_core_gset_pending_members / _commit.
static int gs_ingest_ops_sharded(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                                 uint64_t blob_len, const uint8_t* actors, uint32_t m, const uint32_t* d_fa,
                                 const uint64_t* d_fv, const uint64_t* d_hi, int32_t* status_out) {
  GsGate gt;
  int rc;
  c->pending = false;
  if (!c->has_key) return c->ctx->fail(CE_ERR_NO_KEY, "no latest key");
  if (n) {
    if ((rc = prepare_ingest(c, n, blob_len, actors, m, &gt))) return rc;
  } else {
    // no file on this rank: the windows still set next_op_versions, and the pending batch is
    // empty (no writer needs a slot before the commit)
    hipError_t e;
    if ((c->gs->batch_dirty && (rc = clear_batch(c)))) return rc;
    if ((e = c->ctx->apply.reserve(64))) return c->ctx->hip_fail(e, "ingest reserve");
    writer_versions_of(c, actors, m, &gt.expect);
  }
  // the gate on the device (shard_gate_window): the windows every rank agreed on
  if ((rc = shard_gate_window(c, &c->gs->gate, n, m, d_fa, d_fv, d_hi, &gt.expect, &gt.gap))) return rc;
  if (n && (rc = fold_batch(c, d_blob, d_offs, n, blob_len, status_out))) return rc;
  // pending until the commit: the windows' next_op_versions (lib.rs:537-538)
  c->pending_nov.clear();
  for (uint32_t a = 0; a < m; a++) {
    Uuid u;
    std::memcpy(u.data(), actors + 16ull * a, 16);
    c->pending_nov.push_back({u, gt.expect[a]});
  }
  c->pending = true;
  c->pending_gen = c->table_gen;
  return gt.gap ? CE_ERR_OP_VERSION : CE_OK;
}

}  // namespace ce

using namespace ce;

extern "C" {

int ce_core_gset_ingest_ops_device_sharded(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                                           uint64_t blob_len, const uint8_t* actors, uint32_t m,
                                           const uint32_t* d_fa, const uint64_t* d_fv, const uint64_t* d_hi,
                                           int32_t* status) {
  if (!c || (n && (!d_blob || !d_offs || !d_fa || !d_fv)) || (m && !actors) || !d_hi || c->kind != CE_STATE_GSET)
    return CE_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
  (void)hipSetDevice(c->ctx->device);
  return gs_ingest_ops_sharded(c, d_blob, d_offs, n, blob_len, actors, m, d_fa, d_fv, d_hi, status);
}

int ce_core_gset_apply_bound(uint64_t n, uint32_t per_file, uint32_t* max_files, uint64_t* max_bytes) {
  uint32_t files = 0;
  uint64_t bytes = 0, clear_bound = 0;
  if (!apply_bound(n, &per_file, &files, &bytes, &clear_bound)) return CE_ERR_INVALID_ARG;
  if (max_files) *max_files = files;
  if (max_bytes) *max_bytes = bytes;
  return CE_OK;
}

int ce_core_gset_apply_members_device(ce_core* c, const uint64_t* d_members, uint64_t n, uint32_t per_file,
                                      uint32_t flags, const uint8_t* nonces, uint8_t* d_files, uint64_t cap,
                                      uint64_t* d_file_offs, uint32_t* n_files, uint64_t* bytes) {
  if (!c || (n && !d_members) || !d_file_offs || !n_files || !bytes) return CE_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
  (void)hipSetDevice(c->ctx->device);
  uint32_t max_files = 0;
  uint64_t max_bytes = 0;
  int rc = apply_check(c, n, &per_file, flags, &max_files, &max_bytes);
  if (rc) return rc;
  if (cap < max_bytes || (max_bytes && !d_files))
    return c->ctx->fail(CE_ERR_INVALID_ARG, "gset apply: d_files below ce_core_gset_apply_bound");
  return gs_apply_members_device(c, d_members, n, per_file, flags, nonces, d_files, d_file_offs, n_files, bytes);
}

int ce_core_gset_apply_members(ce_core* c, const uint64_t* members, uint64_t n, uint32_t per_file, uint32_t flags,
                               const uint8_t* nonces, ce_buf* files, ce_buf* file_offs, uint32_t* n_files) {
  if (!c || (n && !members) || !n_files) return CE_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
  (void)hipSetDevice(c->ctx->device);
  ce_ctx* ctx = c->ctx;
  uint32_t max_files = 0;
  uint64_t max_bytes = 0;
  int rc = apply_check(c, n, &per_file, flags, &max_files, &max_bytes);
  if (rc) return rc;
  GsState* g = c->gs;
  hipStream_t s = ctx->stream;
  hipError_t e;
  if ((e = g->up_col.reserve(n * 8 + 64)) || (e = g->up_files.reserve(max_bytes + 64)) ||
      (e = g->up_offs.reserve(8ull * max_files + 64)) ||
      (n && (e = hipMemcpyAsync(g->up_col.p, members, n * 8, hipMemcpyHostToDevice, s))))
    return ctx->hip_fail(e, "gset apply upload");
  uint32_t F = 0;
  uint64_t total = 0;
  if ((rc = gs_apply_members_device(c, g->up_col.as<uint64_t>(), n, per_file, flags, nonces, g->up_files.as<uint8_t>(),
                                    g->up_offs.as<uint64_t>(), &F, &total)))
    return rc;
  std::vector<uint8_t> out;
  std::vector<uint64_t> fo;
  if ((rc = opfile_download(ctx, "gset apply", g->up_files, g->up_offs, total, F, &out, &fo))) return rc;
  fill_files(files, file_offs, out, fo);
  *n_files = F;
  return CE_OK;
}

int ce_core_gset_pending_members(ce_core* c, uint64_t* d_dst, uint64_t cap_members, uint64_t* n) {
  if (!c || !n || c->kind != CE_STATE_GSET) return CE_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
  (void)hipSetDevice(c->ctx->device);
  *n = 0;
  if (!c->pending) return c->ctx->fail(CE_ERR_INVALID_ARG, "no pending batch");
  GsState* g = c->gs;
  hipStream_t s = c->ctx->stream;
  uint32_t hm[kMetaWords];
  int rc = read_meta(c, hm);
  if (rc) return rc;
  *n = (uint64_t)hm[4 + kGsCount] + (hm[4 + kGsZero] ? 1u : 0u);
  if (*n == 0) return CE_OK;
  if (!d_dst || cap_members < *n) return CE_ERR_INVALID_ARG;  // (the size query: *n = what it takes)
  uint32_t* n_out = g->meta.as<uint32_t>() + 15;
  hipError_t e;
  const int t = c->ctx->tbegin("gset_export");
  if ((e = hipMemsetAsync(n_out, 0, 4, s)) ||
      (e = launch_gs_collect(s, batch(g), reinterpret_cast<unsigned long long*>(d_dst), n_out)))
    return c->ctx->hip_fail(e, "gset export");
  c->ctx->tend(t);
  // the caller's collective may run on another stream: the column is complete on return
  if ((e = stream_wait(s))) return c->ctx->hip_fail(e, "gset export");
  return CE_OK;
}

int ce_core_gset_pending_commit(ce_core* c, int accept, const uint64_t* const* d_parts, const uint64_t* counts,
                                uint32_t k) {
  if (!c || c->kind != CE_STATE_GSET) return CE_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
  (void)hipSetDevice(c->ctx->device);
  ce_ctx* ctx = c->ctx;
  if (!c->pending) return ctx->fail(CE_ERR_INVALID_ARG, "no pending batch");
  // the arguments first: a refused call leaves the batch pending
  if (k > kGsMaxParts || (k && (!d_parts || !counts))) return ctx->fail(CE_ERR_INVALID_ARG, "at most 64 parts");
  uint64_t remote = 0;
  for (uint32_t i = 0; i < k; i++) {
    if (counts[i] && !d_parts[i]) return ctx->fail(CE_ERR_INVALID_ARG, "a null part with members");
    if (counts[i] > (1ull << 30) || (remote += counts[i]) > (1ull << 30))
      return ctx->fail(CE_ERR_INVALID_ARG, "set too large for the table");
  }
  GsState* g = c->gs;
  hipStream_t s = ctx->stream;
  c->pending = false;
  if (!accept) return clear_batch(c);  // another rank's batch failed: the state stays unchanged
  uint32_t hm[kMetaWords];
  int rc = read_meta(c, hm);
  if (rc) return rc;
  // grown once, before any insert, to the upper bound (duplicates are unknown): neither the move
  // nor the inserts can meet the load bound
  if ((rc = ensure_committed(c, hm[kGsCount], (uint64_t)hm[4 + kGsCount] + remote))) return rc;
  hipError_t e;
  int t = ctx->tbegin("gset_commit");
  if ((hm[4 + kGsCount] || hm[4 + kGsZero]) && (e = launch_gs_move(s, batch(g), committed(g))))
    return ctx->hip_fail(e, "gset commit");
  ctx->tend(t);
  if (remote) {
    // CE_GSET_PART_LAUNCHES=1: one k_gs_insert launch per part, the form the single launch was
    // measured against (tools/gset_shard_bench.py)
    const char* pl = getenv("CE_GSET_PART_LAUNCHES");
    t = ctx->tbegin("gset_parts");
    if (pl && atoi(pl)) {
      for (uint32_t i = 0; i < k; i++)
        if ((e = launch_gs_insert(s, committed(g), reinterpret_cast<const unsigned long long*>(d_parts[i]),
                                  (uint32_t)counts[i])))
          return ctx->hip_fail(e, "gset commit");
    } else {
      GsParts ps{};
      ps.k = k;
      for (uint32_t i = 0; i < k; i++) {
        ps.part[i] = reinterpret_cast<const unsigned long long*>(d_parts[i]);
        ps.pre[i + 1] = ps.pre[i] + (uint32_t)counts[i];
      }
      if ((e = launch_gs_insert_parts(s, committed(g), ps))) return ctx->hip_fail(e, "gset commit");
    }
    ctx->tend(t);
  }
  if ((rc = clear_batch(c)) || (rc = commit_pending_nov(c))) return rc;
  // the parts are the caller's buffers: read by the time this returns
  if ((e = stream_wait(s))) return ctx->hip_fail(e, "gset commit");
  return CE_OK;
}

}  // extern "C"
