// ce_opfile_host.cpp -- the host steps the op-file writers share (ce_core.h): Core::apply_ops
// (lib.rs:666-722) around each writer's own checks, size and encode kernels and fold.  The writers
// are gs_apply_members_device (ce_gset_host.cpp), ds_add_members_device and ds_rm_members_device
// (ce_dotset_host.cpp).  No step here waits, downloads or allocates beyond what its comment says.
#include <cstring>

#include "ce_core.h"
#include "ce_dotset.h"

namespace ce {

static std::string at(const char* who, const char* step) { return std::string(who) + step; }

void opfile_carve(const ce_core* c, unsigned long long* offs, uint32_t* cols, uint64_t stride, uint64_t* d_file_offs,
                  OpFileLayout* L) {
  L->offs = offs;
  L->clen = cols;
  L->xlen = cols + stride;
  L->coff = cols + 2 * stride;
  L->xoff = cols + 3 * stride;
  L->file_offs = reinterpret_cast<unsigned long long*>(d_file_offs);
  std::memcpy(L->dv, c->current_data_version.data(), 16);
}

int opfile_stage(ce_core* c, const char* who, uint64_t U, const uint8_t* nonces, std::vector<uint8_t>* drawn,
                 OpFileLayout* L) {
  ce_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  hipError_t e;
  const uint64_t F = L->n_files;
  if ((e = ctx->blob.reserve(U + 64)) || (e = ctx->nonces.reserve(24ull * F)) || (e = ctx->outer_ver.reserve(64)))
    return ctx->hip_fail(e, at(who, " reserve").c_str());
  if (!nonces) {
    drawn->resize(24ull * F);
    os_random(drawn->data(), drawn->size());
    nonces = drawn->data();
  }
  L->clear = ctx->blob.as<uint8_t>();
  if ((e = hipMemcpyAsync(ctx->nonces.p, nonces, 24ull * F, hipMemcpyHostToDevice, s)) ||
      (e = hipMemcpyAsync(ctx->outer_ver.p, kCoreVersion, 16, hipMemcpyHostToDevice, s)))
    return ctx->hip_fail(e, at(who, " upload").c_str());
  return CE_OK;
}

hipError_t opfile_scan(const OpFileLayout& L, void* tmp, size_t tmp_bytes, hipStream_t s) {
  size_t tb = tmp_bytes;
  if (hipError_t e = ds_excl_sum_u32(tmp, tb, L.clen, L.coff, L.n_files + 1, s)) return e;
  tb = tmp_bytes;
  return ds_excl_sum_u32(tmp, tb, L.xlen, L.xoff, L.n_files + 1, s);
}

int opfile_seal(ce_core* c, const char* who, const OpFileLayout& L, uint64_t U, uint8_t* d_files, uint64_t* total,
                const unsigned long long* d_word, uint64_t* word) {
  ce_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  hipError_t e;
  const uint64_t* d_file_offs = reinterpret_cast<const uint64_t*>(L.file_offs);
  // file i = CURRENT_VERSION || Cryptor::encrypt(clear_i) (lib.rs:682-695), straight into d_files
  if (int rc = device_seal(ctx, L.clear, reinterpret_cast<const uint64_t*>(L.offs), L.n_files, U,
                           ctx->outer_ver.as<uint8_t>(), ctx->nonces.as<uint8_t>(), d_files, d_file_offs, key_of(c)))
    return rc;
  if ((e = hipMemcpyAsync(total, d_file_offs + L.n_files, 8, hipMemcpyDeviceToHost, s)) ||
      (d_word && (e = hipMemcpyAsync(word, d_word, 8, hipMemcpyDeviceToHost, s))) || (e = stream_wait(s)))
    return ctx->hip_fail(e, who);
  return CE_OK;
}

int opfile_store(ce_core* c, const char* who, const OpFileLayout& L, const uint8_t* d_files, uint64_t total, uint64_t* v0) {
  ce_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  hipError_t e;
  const uint32_t F = L.n_files;
  uint32_t slot;
  if (int rc = insert_actor(c, c->local_actor, &slot)) return rc;
  *v0 = c->nov[slot];  // next_op_versions.get(actor) (lib.rs:703)
  if (!c->storage) return CE_OK;
  std::vector<uint8_t> out(total);
  std::vector<uint64_t> fo(F + 1);
  if ((e = hipMemcpyAsync(out.data(), d_files, total, hipMemcpyDeviceToHost, s)) ||
      (e = hipMemcpyAsync(fo.data(), L.file_offs, 8ull * (F + 1), hipMemcpyDeviceToHost, s)) || (e = stream_wait(s)))
    return ctx->hip_fail(e, at(who, " download").c_str());
  for (uint32_t i = 0; i < F; i++)
    if (int rc = storage_store_op(c->storage, c->local_actor, *v0 + i, out.data() + fo[i], fo[i + 1] - fo[i]))
      return ctx->fail(rc, "failed writing ops file");
  return CE_OK;
}

int opfile_finish(ce_core* c, uint64_t v0, uint32_t F) {
  c->nov[c->slot_of.at(c->local_actor)] = v0 + F;  // next_op_versions.inc(actor), once a file (lib.rs:714-715)
  return table_upload(c);
}

int opfile_empty(ce_core* c, const char* who, uint64_t* d_file_offs, uint32_t* n_files, uint64_t* bytes) {
  hipStream_t s = c->ctx->stream;
  hipError_t e;
  if (d_file_offs && ((e = hipMemsetAsync(d_file_offs, 0, 8, s)) || (e = stream_wait(s)))) return c->ctx->hip_fail(e, who);
  *n_files = 0;
  *bytes = 0;
  return CE_OK;
}

int opfile_download(ce_ctx* ctx, const char* who, const DevBuf& files, const DevBuf& offs, uint64_t total, uint32_t F,
                    std::vector<uint8_t>* out, std::vector<uint64_t>* fo) {
  hipStream_t s = ctx->stream;
  hipError_t e;
  out->resize(total);
  fo->resize(F + 1);
  if ((total && (e = hipMemcpyAsync(out->data(), files.p, total, hipMemcpyDeviceToHost, s))) ||
      (e = hipMemcpyAsync(fo->data(), offs.p, 8ull * (F + 1), hipMemcpyDeviceToHost, s)) || (e = stream_wait(s)))
    return ctx->hip_fail(e, at(who, " download").c_str());
  return CE_OK;
}

void fill_buf(ce_buf* out, const void* p, size_t n) {
  out->data = (uint8_t*)malloc(n ? n : 1);
  if (n) std::memcpy(out->data, p, n);
  out->len = n;
}

void fill_files(ce_buf* files, ce_buf* file_offs, const std::vector<uint8_t>& out, const std::vector<uint64_t>& fo) {
  if (files) fill_buf(files, out.data(), out.size());
  if (file_offs) fill_buf(file_offs, fo.data(), fo.size() * 8);
}

}  // namespace ce
