// ce_lww_host.cpp -- Core<LWWReg<u64, u64>> (CE_STATE_LWWREG): the host side.  Same contracts as
// the VClock / GCounter paths in ce_core.cpp.
//
// The committed register (val, marker) is two words on the host.  An ingest opens, checks and
// decodes every file on the device: single-page files in the fused open (ce_fused.hip
// k_open_fold_v3's LW form, plaintext in LDS), larger files, host-parse envelopes and multi-key
// retries from HBM by k_decode_lww.  Either leaves the file's own winner in a per-file record
// column (ce_lww.h); the host reads the statuses, and only when every file passed does k_lww_reduce
// pick the batch's winner and the host apply LWWReg::update to the register: a failing batch
// leaves the register and next_op_versions as they were (all-or-nothing, lib.rs:497-514).
//
// Ties: a marker equal to the register's changes nothing; among the batch's ops with the largest
// marker the first in apply order wins (lowest file index, then lowest index in its file:
// read_remote_ops keeps the batch's order).  State files and merge_state are parsed on the host
// and applied in call order -- the reference merges states in completion order and so leaves a tie
// between two of them unspecified.
//
// The sharded ingest (ce_core_lwwreg_ingest_ops_device_sharded, at the end of this file): a rank
// opens and decodes its share of a batch partitioned by op-file address in the same way, gates it
// on the device by the agreed windows, and keeps its winner PENDING with the file's (writer index,
// version), its place in the whole batch's apply order; ce_core_lwwreg_pending_commit applies the
// best of the ranks' winners in that order, which is the single fold's winner.
#include <algorithm>
#include <cstring>

#include "ce_core.h"
#include "ce_lww.h"

namespace ce {

struct LwState {
  uint64_t val = 0, marker = 0;  // the committed register
  DevBuf rec;                    // LwwRec[n]: the batch's per-file records
  DevBuf red;                    // LwwPartial[kLwwMaxBlocks] | LwwRec (the result) | paths u32[4]
  DevBuf fused;                  // LwwFused: what the fused open reads through DecodeArgs.lw
  LwwFused h_fused;              // its host copy (lives through the upload)
  DevBuf only;
  // the sharded ingest: the window gate's block, the keyed reduce's scratch and the share's
  // winner, pending (with ce_core.pending / pending_nov) until ce_core_lwwreg_pending_commit
  DevBuf gate;                   // e0 u64[m] | newnov u64[m]
  DevBuf kred;                   // LwwKeyedPartial[kLwwMaxBlocks] | LwwKeyed (the result)
  LwwKeyed pend = kLwwKeyedNone;
};

void lw_free(LwState* l) { delete l; }

namespace {

constexpr uint64_t kResultAt = sizeof(LwwPartial) * kLwwMaxBlocks;
constexpr uint64_t kPathsAt = kResultAt + sizeof(LwwRec);

LwwRec* result_of(LwState* l) { return reinterpret_cast<LwwRec*>(l->red.as<uint8_t>() + kResultAt); }
uint32_t* paths_of(LwState* l) { return reinterpret_cast<uint32_t*>(l->red.as<uint8_t>() + kPathsAt); }

// LWWReg::update
void update(LwState* l, uint64_t val, uint64_t marker) {
  if (l->marker < marker) {
    l->val = val;
    l->marker = marker;
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

// decode the files of `only` (null: all; large_only: those of more than one page) from their
// plaintext in HBM into their rows of the record column
int decode_pass(ce_core* c, uint32_t n, const uint8_t* only, bool large_only = false) {
  ce_ctx* ctx = c->ctx;
  LwState* l = c->lw;
  hipError_t e;
  LwwDecodeArgs a{};
  a.pt = ctx->out.as<uint8_t>();
  a.params = ctx->params.as<FileParams>();
  a.status = ctx->status.as<int32_t>();
  a.n = n;
  a.supported = c->d_supported.as<uint8_t>();
  a.n_supported = (uint32_t)c->supported.size();
  a.apply = ctx->apply.as<uint8_t>();
  a.only = only;
  a.large_only = large_only ? 1 : 0;
  a.rec = l->rec.as<LwwRec>();
  a.paths = paths_of(l);
  uint32_t hp[4];
  if ((e = hipMemsetAsync(a.paths, 0, 16, ctx->stream))) return ctx->hip_fail(e, "lww decode");
  const int t = ctx->tbegin("decode_lww");
  if ((e = launch_decode_lww(ctx->stream, a, grid_waves_for(n)))) return ctx->hip_fail(e, "lww decode");
  ctx->tend(t);
  if ((e = hipMemcpyAsync(hp, a.paths, 16, hipMemcpyDeviceToHost, ctx->stream)) || (e = stream_wait(ctx->stream)))
    return ctx->hip_fail(e, "lww decode");
  c->path_counts["lww_uniform_files"] += hp[0];
  c->path_counts["lww_general_files"] += hp[1];
  c->path_counts["lww_page_files"] += hp[3];
  return CE_OK;
}

bool read_reg(Rd& r, uint64_t* val, uint64_t* marker) { return parse_lww_op(r, val, marker) == 1; }

struct LwGate {
  std::vector<uint32_t> wslot;
  uint64_t gen0 = 0;
  std::vector<uint64_t> expect;
  uint32_t first_gap = 0xffffffffu;  // the file at the gap (n: none)
};

// writers get slots first (the gate is keyed by them); the batch's scratch
int prepare_ingest(ce_core* c, uint32_t n, uint64_t blob_len, const uint8_t* actors, uint32_t m, LwGate* gt) {
  ce_ctx* ctx = c->ctx;
  LwState* l = c->lw;
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
      (e = ctx->apply.reserve(n + 64)) || (e = l->only.reserve(n + 64)) ||
      (e = l->rec.reserve(sizeof(LwwRec) * (uint64_t)n + 64)) || (e = l->red.reserve(kPathsAt + 64)) ||
      (e = l->fused.reserve(sizeof(LwwFused))))
    return ctx->hip_fail(e, "ingest reserve");
  gt->expect.resize(m);
  for (uint32_t a = 0; a < m; a++) gt->expect[a] = c->nov[gt->wslot[a]];
  return CE_OK;
}

// the version gate (lib.rs:519-538) on the host: it needs no plaintext
int gate_host(ce_core* c, uint32_t n, uint32_t m, const uint32_t* d_fa, const uint64_t* d_fv, LwGate* gt) {
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

// Every file opened, checked and decoded whatever the gate says; the gated files' winners
// (apply[], already on the device) into their rows of the record column.  A failing file: its
// status is returned (the lowest failing file's) and the column is not to be reduced.  Shared by
// the unsharded and the sharded ingest.
int open_decode(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n, uint64_t blob_len,
                int32_t* status_out) {
  ce_ctx* ctx = c->ctx;
  LwState* l = c->lw;
  hipError_t e;
  int rc;
  // single-page files: opened, checked and decoded in one kernel, the plaintext in LDS
  // (k_open_fold_v3's LW form, lib.rs:501-507); larger files: opened to HBM by the segment pass
  // and decoded whole by k_decode_lww
  uint32_t ec = 0;
  if ((rc = device_open_setup(ctx, d_blob, d_offs, n, blob_len, true, key_of(c), ctx->status.as<int32_t>(), &ec)))
    return rc;
  uint32_t* paths = paths_of(l);
  l->h_fused = LwwFused{l->rec.as<LwwRec>(), paths};
  if ((e = hipMemsetAsync(l->rec.p, 0, sizeof(LwwRec) * (uint64_t)n, ctx->stream)) ||
      (e = hipMemsetAsync(paths, 0, 16, ctx->stream)) ||
      (e = hipMemcpyAsync(l->fused.p, &l->h_fused, sizeof(LwwFused), hipMemcpyHostToDevice, ctx->stream)))
    return ctx->hip_fail(e, "lww fused args");
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
  da.lw = l->fused.as<LwwFused>();
  ctx->open_log.grid_cap = test_grid_cap();
  ctx->open_log.stamps = test_wave_stamps(ctx);
  ctx->open_log.stamp_waves = 0;  // this ingest's launches, if stamped, are the ones to read
  {
    hipEvent_t t0, t1;
    (void)ctx->tlaunch("open_fold_small", &t0, &t1);
    if ((e = launch_open_fold_lww(ctx->stream, da, ctx->open_log, t0, t1))) return ctx->hip_fail(e, "fused");
  }
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
  uint32_t hp[4], hc[16];
  if ((e = hipMemcpyAsync(hc, ctx->counters.p, 64, hipMemcpyDeviceToHost, ctx->stream)) ||
      (e = hipMemcpyAsync(hp, paths, 16, hipMemcpyDeviceToHost, ctx->stream)) || (e = stream_wait(ctx->stream)))
    return ctx->hip_fail(e, "counters");
  c->path_counts["lww_uniform_files"] += hp[0];
  c->path_counts["lww_general_files"] += hp[1];
  c->path_counts["lww_fused_files"] += hp[2];
  if (hc[9] && (rc = decode_pass(c, n, nullptr, true))) return rc;  // files of more than one page
  std::vector<int32_t> st;
  if ((rc = download_status(c, n, &st))) return rc;
  if (std::find(st.begin(), st.end(), kStatusHostParse) != st.end()) {
    // envelopes left to the host: opened there, the plaintext patched into HBM, decoded from it
    std::vector<uint8_t> sel(n);
    for (uint32_t i = 0; i < n; i++) sel[i] = st[i] == kStatusHostParse;
    if ((rc = resolve_host_parse(c, d_blob, d_offs, n, true))) return rc;
    if ((e = hipMemcpyAsync(l->only.p, sel.data(), n, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = stream_wait(ctx->stream)))
      return ctx->hip_fail(e, "host parse mask");
    if ((rc = decode_pass(c, n, l->only.as<uint8_t>())) || (rc = download_status(c, n, &st))) return rc;
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
        if ((e = hipMemcpyAsync(l->only.p, sel.data(), n, hipMemcpyHostToDevice, ctx->stream)) ||
            (e = stream_wait(ctx->stream)))
          return ctx->hip_fail(e, "multi-key mask");
        if ((rc = decode_pass(c, n, l->only.as<uint8_t>())) || (rc = download_status(c, n, &sk))) return rc;
        for (uint32_t i = 0; i < n; i++)
          if (sel[i]) st[i] = sk[i];
      }
    }
  }
  if (status_out) std::memcpy(status_out, st.data(), n * 4ull);
  for (uint32_t i = 0; i < n; i++)
    if (st[i] != CE_OK) return st[i];  // all-or-nothing: the register is untouched
  return CE_OK;
}

// open_decode, then the batch's winner by (marker descending, file index ascending); *win: (0, 0)
// for none
int fold_batch(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n, uint64_t blob_len,
               int32_t* status_out, LwwRec* win) {
  ce_ctx* ctx = c->ctx;
  LwState* l = c->lw;
  hipError_t e;
  int rc;
  if ((rc = open_decode(c, d_blob, d_offs, n, blob_len, status_out))) return rc;
  // the batch's winner: largest marker, lowest file index
  const int t = ctx->tbegin("lww_reduce");
  if ((e = launch_lww_reduce(ctx->stream, l->rec.as<LwwRec>(), n, l->red.as<LwwPartial>(), result_of(l),
                             test_grid_cap())))
    return ctx->hip_fail(e, "lww reduce");
  ctx->tend(t);
  if ((e = hipMemcpyAsync(win, result_of(l), sizeof(LwwRec), hipMemcpyDeviceToHost, ctx->stream)) ||
      (e = stream_wait(ctx->stream)))
    return ctx->hip_fail(e, "lww reduce");
  return CE_OK;
}

}  // namespace

bool parse_lww_ops(const uint8_t* p, size_t n, std::vector<uint64_t>* out) {
  Rd r{p, n, 0};
  uint64_t cnt;
  if (!rd_array_hdr(r, &cnt) || cnt > r.n - r.i) return false;  // each element takes >= 1 byte
  for (uint64_t k = 0; k < cnt; k++) {
    uint64_t v = 0, m = 0;
    if (!read_reg(r, &v, &m)) return false;  // (too deep for the bounded skip: rejected)
    out->push_back(v);
    out->push_back(m);
  }
  return true;
}

bool read_lww_state(Rd& r, std::vector<uint64_t>* out) {
  uint64_t v = 0, m = 0;
  if (!read_reg(r, &v, &m)) return false;
  out->push_back(v);
  out->push_back(m);
  return true;
}

void write_lww_state(ce_core* c, Wr* w) {
  w->map(2);
  w->str("val");
  w->uint(c->lw->val);
  w->str("marker");
  w->uint(c->lw->marker);
}

int lw_init(ce_core* c) {
  c->lw = new LwState();
  // what the reduce's tests place their ties around (ce_lww.h)
  c->path_counts["lww_reduce_tile"] = kLwwTile;
  c->path_counts["lww_reduce_max_blocks"] = kLwwMaxBlocks;
  return CE_OK;
}

int lw_reset(ce_core* c) {
  c->lw->val = c->lw->marker = 0;
  c->pending = false;  // a pending sharded batch goes with the register
  return CE_OK;
}

void lw_apply_pairs(ce_core* c, const std::vector<uint64_t>& pairs) {
  for (size_t i = 0; i + 1 < pairs.size(); i += 2) update(c->lw, pairs[i], pairs[i + 1]);
}

void lw_read(ce_core* c, uint64_t* val, uint64_t* marker) {
  *val = c->lw->val;
  *marker = c->lw->marker;
}

int lw_ingest_ops(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n, uint64_t blob_len,
                  const uint8_t* actors, uint32_t m, const uint32_t* d_fa, const uint64_t* d_fv,
                  int32_t* status_out) {
  LwGate gt;
  LwwRec win{0, 0};
  int rc;
  if ((rc = prepare_ingest(c, n, blob_len, actors, m, &gt)) || (rc = gate_host(c, n, m, d_fa, d_fv, &gt)) ||
      (rc = fold_batch(c, d_blob, d_offs, n, blob_len, status_out, &win)))
    return rc;
  // commit, next_op_versions (lib.rs:537-538) and the gap error (lib.rs:527-531)
  update(c->lw, win.val, win.marker);
  if (c->table_gen != gt.gen0) refresh_slots(c, actors, m, &gt.wslot);
  for (uint32_t w = 0; w < m; w++) c->nov[gt.wslot[w]] = std::max(c->nov[gt.wslot[w]], gt.expect[w]);
  if (gt.first_gap < n) {
    if (status_out) status_out[gt.first_gap] = CE_ERR_OP_VERSION;
    return CE_ERR_OP_VERSION;
  }
  return CE_OK;
}

// The sharded ingest (crdtenc shard.ingest_lwwreg_sharded): the same open and decode with the
// agreed windows as the gate, the share's winner left PENDING with its address (writer index in
// the shared list, version) for ce_core_lwwreg_pending_record / _commit.
static int lw_ingest_ops_sharded(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                                 uint64_t blob_len, const uint8_t* actors, uint32_t m, const uint32_t* d_fa,
                                 const uint64_t* d_fv, const uint64_t* d_hi, int32_t* status_out) {
  ce_ctx* ctx = c->ctx;
  LwState* l = c->lw;
  LwGate gt;
  hipError_t e;
  int rc;
  bool gap = false;
  c->pending = false;
  if (!c->has_key) return ctx->fail(CE_ERR_NO_KEY, "no latest key");
  if (n) {
    if ((rc = prepare_ingest(c, n, blob_len, actors, m, &gt))) return rc;
  } else {
    // no file on this rank: the windows still set next_op_versions, and the pending record is
    // "none" (no writer needs a slot before the commit)
    if ((e = ctx->apply.reserve(64))) return ctx->hip_fail(e, "ingest reserve");
    writer_versions_of(c, actors, m, &gt.expect);
  }
  if ((rc = shard_gate_window(c, &l->gate, n, m, d_fa, d_fv, d_hi, &gt.expect, &gap))) return rc;
  LwwKeyed win = kLwwKeyedNone;
  if (n) {
    if ((rc = open_decode(c, d_blob, d_offs, n, blob_len, status_out))) return rc;
    // the share's winner: largest marker, then the earliest (writer, version) of the whole batch
    constexpr uint64_t kOutAt = sizeof(LwwKeyedPartial) * kLwwMaxBlocks;
    if ((e = l->kred.reserve(kOutAt + sizeof(LwwKeyed)))) return ctx->hip_fail(e, "lww reduce");
    LwwKeyed* out = reinterpret_cast<LwwKeyed*>(l->kred.as<uint8_t>() + kOutAt);
    const int t = ctx->tbegin("lww_reduce");
    if ((e = launch_lww_reduce_keyed(ctx->stream, l->rec.as<LwwRec>(), d_fa, d_fv, n, l->kred.as<LwwKeyedPartial>(),
                                     out, test_grid_cap())))
      return ctx->hip_fail(e, "lww reduce");
    ctx->tend(t);
    if ((e = hipMemcpyAsync(&win, out, sizeof(LwwKeyed), hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = stream_wait(ctx->stream)))
      return ctx->hip_fail(e, "lww reduce");
  }
  // pending until the commit: the winner and the windows' next_op_versions (lib.rs:537-538)
  l->pend = win;
  c->pending_nov.clear();
  for (uint32_t a = 0; a < m; a++) {
    Uuid u;
    std::memcpy(u.data(), actors + 16ull * a, 16);
    c->pending_nov.push_back({u, gt.expect[a]});
  }
  c->pending = true;
  c->pending_gen = c->table_gen;
  return gap ? CE_ERR_OP_VERSION : CE_OK;
}

}  // namespace ce

using namespace ce;

extern "C" {

int ce_core_lwwreg_ingest_ops_device_sharded(ce_core* c, const uint8_t* d_blob, const uint64_t* d_offs, uint32_t n,
                                             uint64_t blob_len, const uint8_t* actors, uint32_t m,
                                             const uint32_t* d_fa, const uint64_t* d_fv, const uint64_t* d_hi,
                                             int32_t* status) {
  if (!c || (n && (!d_blob || !d_offs || !d_fa || !d_fv)) || (m && !actors) || !d_hi || c->kind != CE_STATE_LWWREG)
    return CE_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
  (void)hipSetDevice(c->ctx->device);
  return lw_ingest_ops_sharded(c, d_blob, d_offs, n, blob_len, actors, m, d_fa, d_fv, d_hi, status);
}

int ce_core_lwwreg_pending_record(ce_core* c, uint64_t rec[4]) {
  if (!c || !rec || c->kind != CE_STATE_LWWREG) return CE_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
  if (!c->pending) return c->ctx->fail(CE_ERR_INVALID_ARG, "no pending batch");
  const LwwKeyed& w = c->lw->pend;
  rec[0] = w.marker;
  rec[1] = w.val;
  rec[2] = w.fa;
  rec[3] = w.fv;
  return CE_OK;
}

int ce_core_lwwreg_pending_commit(ce_core* c, int accept, const uint64_t* recs, uint32_t k) {
  if (!c || c->kind != CE_STATE_LWWREG) return CE_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
  (void)hipSetDevice(c->ctx->device);
  ce_ctx* ctx = c->ctx;
  // the arguments first: a refused call leaves the batch pending
  if (k > 64 || (k && !recs)) return ctx->fail(CE_ERR_INVALID_ARG, "at most 64 remote records");
  if (!c->pending) return ctx->fail(CE_ERR_INVALID_ARG, "no pending batch");
  c->pending = false;
  if (!accept) return CE_OK;  // another rank's batch failed: the state stays unchanged
  // the whole batch's winner: the best of the shares' winners in the batch's apply order
  LwwKeyed best = c->lw->pend;
  for (uint32_t i = 0; i < k; i++) {
    const uint64_t* r = recs + 4ull * i;
    if (r[0] && lww_keyed_better(r[0], r[2], r[3], 0, best.marker, best.fa, best.fv, 0))
      best = LwwKeyed{r[0], r[1], r[2], r[3]};
  }
  if (best.marker) update(c->lw, best.val, best.marker);  // (a tie with the register keeps the incumbent)
  return commit_pending_nov(c);
}

}  // extern "C"
