// ce_opfile.h -- what the op-file writers share, host and device: the GSet writer
// (ce_gset_write.hip), the Orswot add-op writer (ce_orswot_write.hip) and the Orswot Rm-op writer
// (ce_orswot_rm.hip).
//
// Each lays a member column in HBM out as many small op files.  File i's clear text is
// VersionBytes(data_version, to_vec_named(Vec<Op>)) (crdt-enc/src/lib.rs:670-671): 16 bytes of
// data version, an array header, the ops, every integer big-endian in its smallest unsigned form.
// A size pass writes clen / xlen, two scans give coff / xoff, an encoder writes the clear texts
// back to back and the two offset columns device_seal reads.  The device pieces are in
// ce_opfile_device.h, the host steps in ce_opfile_host.cpp (declared in ce_core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_common.h"

namespace ce {

// the least a sealed file adds to its clear text: the outer version and an envelope whose two bin
// headers are bin8
static constexpr uint64_t kOpFileSealBase = 16 + sealed_len(0);

struct OpFileLayout {
  uint32_t n_files;
  uint32_t* clen;              // [n_files + 1] clear lengths, clen[n_files] = 0 (the size pass)
  uint32_t* xlen;              // [n_files + 1] a sealed file's bytes past its clear text and kOpFileSealBase
  uint32_t* coff;              // [n_files + 1] exclusive sums of clen (the encoder reads them)
  uint32_t* xoff;              //               and of xlen
  uint8_t dv[16];              // the data version
  uint8_t* clear;              // the clear texts back to back, 16-byte aligned
  unsigned long long* offs;    // [n_files + 1] clear offsets for the seal
  unsigned long long* file_offs;  // [n_files + 1] sealed offsets: coff + i * kOpFileSealBase + xoff
};

// header lengths: an array of cnt < 65536 elements, a map of k entries
CE_HD constexpr uint32_t arr_hdr_len(uint32_t cnt) { return cnt <= 15 ? 1u : 3u; }
CE_HD constexpr uint32_t rm_map_hdr(uint32_t k) { return k <= 15 ? 1u : k <= 65535 ? 3u : 5u; }
// byte k of an array header of hc = arr_hdr_len(cnt) bytes (fixarray, array16)
CE_HD uint8_t arr_hdr_byte(uint32_t cnt, uint32_t hc, uint32_t k) {
  if (hc == 1) return (uint8_t)(0x90 | cnt);
  return k == 0 ? (uint8_t)0xdc : k == 1 ? (uint8_t)(cnt >> 8) : (uint8_t)cnt;
}

// an unsigned integer's smallest form (fixint, cc, cd, ce, cf): its length, byte k of it
// (wd = uint_width(v)), and the whole of it at p
CE_HD uint32_t uint_width(unsigned long long v) {
  return v <= 0x7f ? 1u : v <= 0xff ? 2u : v <= 0xffff ? 3u : v <= 0xffffffffull ? 5u : 9u;
}
CE_HD uint8_t uint_byte(unsigned long long v, uint32_t wd, uint32_t k) {
  if (k == 0) return wd == 1 ? (uint8_t)v : (uint8_t)(wd == 2 ? 0xcc : wd == 3 ? 0xcd : wd == 5 ? 0xce : 0xcf);
  return (uint8_t)(v >> (8 * (wd - 1 - k)));
}
CE_HD uint32_t put_uint(uint8_t* p, unsigned long long v) {
  const uint32_t wd = uint_width(v);
  for (uint32_t k = 0; k < wd; k++) p[k] = uint_byte(v, wd, k);
  return wd;
}

// blocks of per_block units of work, at least one and at most cap
inline uint32_t grid_blocks(uint64_t work, uint32_t per_block, uint32_t cap) {
  const uint64_t b = (work + per_block - 1) / per_block;
  return b < 1 ? 1u : (b > cap ? cap : (uint32_t)b);
}

// The file size pass of a writer whose files are runs of opf ops (the last may hold fewer), a lane
// per file: clen / xlen from ooff, the exclusive sums of the n_ops ops' byte lengths;
// clen[n_files] = xlen[n_files] = 0 (ce_opfile.hip)
hipError_t launch_opfile_sizes(hipStream_t s, const OpFileLayout& L, const uint32_t* ooff, uint32_t opf, uint32_t n_ops);

}  // namespace ce
