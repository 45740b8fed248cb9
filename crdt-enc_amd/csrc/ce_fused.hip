// ce_fused.hip -- the C2 hot loop: open + decode + fold of single-page op files in one kernel,
// and the device version gate.
//
// k_open_fold_small<LPF>: a wavefront handles 64/LPF files at once, LPF lanes per file.
//   1. the file's ciphertext pieces (16 B, coalesced per file) are loaded into registers first,
//      so their latency hides under step 2;
//   2. each lane computes 64/LPF ChaCha20 blocks of the page (counter 1 + block) into LDS;
//   3. piece by piece: keystream from LDS (transposed), plaintext written back over the
//      consumed keystream (LDS), Poly1305 as an LPF-way strided Horner in r^LPF;
//   4. log2(LPF)-level cross-lane tree in r^(2^k) inside the lane group, tag compare
//      (xchacha lib.rs:92-97) -- a failing file folds nothing;
//   5. the plaintext never leaves LDS: VersionBytes data-version check (crdt-enc/src/lib.rs:
//      504-505) and rmp-serde Vec<Dot<Uuid>> decode (lib.rs:507), LPF candidate Dots per round
//      speculating on the canonical encoding (general grammar by the group leader otherwise);
//   6. dots of files the gate applies are max-folded into the batch state (VClock::apply),
//      one pending (slot, max) per lane group -> one atomicMax per file for an actor's own ops.
// Poly1305 tree cost per file falls from 7 mulmods (64 lanes/file) to 5/4 (16 lanes/file).
#include <algorithm>

#include <hip/hip_ext.h>

#include "ce_device.h"
#include "ce_gset_device.h"
#include "ce_lww.h"

namespace ce {

// LDS per file in flight: 64 keystream blocks at an 80-byte stride (5120 B).  Any padding
// beyond this costs resident blocks: 4 x (2 waves x 4 files x 5120 B) is exactly 160 KiB.
// Regions are packed at a 5104-byte stride: the last keystream block's 16 pad bytes are never
// touched, so neighbouring regions may overlap them.  5104 B = 1276 dwords = -4 (mod 64 banks):
// the four files of a wave sit on different banks at equal offsets (their decode reads would
// otherwise collide 4-way), and 8 regions still fit 40 KiB per 2-wave block (4 blocks/CU).
static constexpr uint32_t kRegion = 64 * kKsStride - 16;

#ifndef CE_NCH
#define CE_NCH 2
#endif
template <int LPF>
struct FusedCfg {
  static constexpr int F = 64 / LPF;                       // files per wave
  static constexpr int WPB = LPF == 16 ? 2 : 4;            // waves per block
  static constexpr int LOG = LPF == 16 ? 4 : LPF == 32 ? 5 : 6;
  static constexpr int WAVES_PER_SIMD = LPF == 16 ? 2 : LPF == 32 ? 3 : 4;  // LDS-limited
  // independent Horner chains per lane: chain c takes the lane's slots t = c mod NCH and steps
  // by r^(LPF * NCH) (FileParams.rpow[LOG + LOGCH]) -- NCH-way ILP on the mulmod dependency
  // chain for one extra mulmod per chain to combine them
  static constexpr int NCH = LPF * CE_NCH <= 64 ? CE_NCH : 64 / LPF;  // step r^(LPF NCH) <= r^64
  static constexpr int LOGCH = NCH == 4 ? 2 : NCH == 2 ? 1 : 0;
};

// ---- lane-group collectives (a group = the LPF lanes of one file) --------------------------
// DPP inside a row of 16 lanes (no LDS round trip); wider groups add xor-shuffles.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
// lane i <- lane i + d inside the row (0 past the row's end), d in {1, 2, 4, 8}
__device__ __forceinline__ uint32_t row_down(uint32_t v, int d) {
  switch (d) {
    case 1: return dpp<0x101>(v);
    case 2: return dpp<0x102>(v);
    case 4: return dpp<0x104>(v);
    default: return dpp<0x108>(v);
  }
}
template <int LPF, typename Op>
__device__ __forceinline__ uint32_t grp_reduce(uint32_t v, Op op) {
  v = op(v, dpp<0xB1>(v));   // quad_perm [1,0,3,2]
  v = op(v, dpp<0x4E>(v));   // quad_perm [2,3,0,1]
  v = op(v, dpp<0x141>(v));  // row_half_mirror
  v = op(v, dpp<0x140>(v));  // row_mirror
  if (LPF >= 32) v = op(v, (uint32_t)__shfl_xor((int)v, 16));
  if (LPF >= 64) v = op(v, (uint32_t)__shfl_xor((int)v, 32));
  return v;
}
template <int LPF>
__device__ __forceinline__ unsigned long long grp_max64(unsigned long long v) {
  auto step = [&](uint32_t lo, uint32_t hi) {
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o > v ? o : v;
  };
  step(dpp<0xB1>((uint32_t)v), dpp<0xB1>((uint32_t)(v >> 32)));
  step(dpp<0x4E>((uint32_t)v), dpp<0x4E>((uint32_t)(v >> 32)));
  step(dpp<0x141>((uint32_t)v), dpp<0x141>((uint32_t)(v >> 32)));
  step(dpp<0x140>((uint32_t)v), dpp<0x140>((uint32_t)(v >> 32)));
  if (LPF >= 32) step((uint32_t)__shfl_xor((int)(uint32_t)v, 16), (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), 16));
  if (LPF >= 64) step((uint32_t)__shfl_xor((int)(uint32_t)v, 32), (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), 32));
  return v;
}
// failure counters of the wave's rejected files (counters[2] += count, counters[5] = min file
// index), accumulated wave-uniformly over the grid-stride loop and added once per wave at the
// end (AuthFails::flush).  Same-address atomics serialise in one L2 channel: per file or even
// per wave-iteration they cost ~1 ms when half of 1M files are rejected (C5).  The lowest set
// lane of a ballot holds the iteration's lowest failing index (file = g * F + lane group).
struct AuthFails {
  uint32_t n = 0, fmin = 0xffffffffu;
  __device__ __forceinline__ void add(bool failed, uint32_t f) {
    const unsigned long long bm = __ballot(failed);
    if (bm) {
      n += (uint32_t)__builtin_popcountll(bm);
      const uint32_t f0 = (uint32_t)__shfl((int)f, (int)__builtin_ctzll(bm));
      fmin = f0 < fmin ? f0 : fmin;
    }
  }
  __device__ __forceinline__ void flush(const DecodeArgs& a) const {
    if (n && (threadIdx.x & 63) == 0) {
      atomicAdd(&a.counters[2], n);
      atomicMin(&a.counters[5], fmin);
    }
  }
};

// this lane's group bit of a wave ballot
template <int LPF>
__device__ __forceinline__ unsigned long long grp_bits(bool p, uint32_t grp) {
  constexpr unsigned long long GM = LPF == 64 ? ~0ull : ((1ull << LPF) - 1);
  return (__ballot(p) >> (grp * LPF)) & GM;
}

// canonical Dot lengths <-> 3-bit codes (ballot transport of the next Dot's length), branch-free:
// L - 34 in {0, 1, 2, 4, 8} -> code 1..5 through a nibble table; anything else -> 0
__device__ __forceinline__ uint32_t len_code(uint32_t L) {
  const uint32_t d = L - 34u;
  return d < 16u ? (uint32_t)((0x500040321ull >> (4u * d)) & 0xfu) : 0u;
}
// code 1..5 -> 34 + {0, 1, 2, 4, 8}
__device__ __forceinline__ uint32_t code_len(uint32_t c) { return 34u + ((1u << c) >> 2); }

// per-iteration inputs of one file, prefetched one grid-stride iteration ahead
struct FilePre {
  uint32_t ok;      // file exists, selected, setup status OK
  uint32_t apply;   // version gate lets this file fold
  uint32_t len;
  uint32_t in_off;  // ciphertext offset in the blob (lo, hi)
  uint32_t in_hi;
  uint32_t key[8];
  uint32_t n2a, n2b;
  uint32_t R[5];    // r^(LPF * NCH): the Horner step of every chain
};

template <int RIDX>
__device__ __forceinline__ FilePre load_pre(const DecodeArgs& a, uint32_t f) {
  FilePre p;
  const bool in = f < a.n;
  const uint32_t fi = in ? f : 0u;
  const FileParams* Pp = a.params + fi;
  // status, only and apply are independent loads: no per-lane short circuit (that would wait
  // for each before issuing the next)
  const int32_t stv = a.status[fi];
  const uint32_t ov = a.only ? (uint32_t)a.only[fi] : 1u;
  const uint32_t av = a.apply ? (uint32_t)a.apply[fi] : 1u;
  p.ok = (uint32_t)in & (uint32_t)(stv == CE_OK) & (uint32_t)(ov != 0);
  p.apply = av != 0;
  p.len = Pp->len;
  p.in_off = (uint32_t)Pp->in_off;
  p.in_hi = (uint32_t)(Pp->in_off >> 32);
#pragma unroll
  for (int i = 0; i < 8; i++) p.key[i] = Pp->subkey[i];
  p.n2a = Pp->n2[0];
  p.n2b = Pp->n2[1];
#pragma unroll
  for (int i = 0; i < 5; i++) p.R[i] = Pp->rpow[RIDX][i];
  return p;
}

// decode state a lane group carries from file to file: speculated Dot length, actor cache
struct DecState {
  uint32_t Ls;
  uint32_t ck0, ck1, ck2, ck3, cslot;
  // CARRY (k_open_fold_v3): the lane's pending (slot, max) carried from file to file -- a wave
  // takes a contiguous run of files, a writer's run, so one flush per writer instead of per file
  uint32_t pslot = 0xffffffffu;
  unsigned long long pbest = 0;
};

// one atomicMax per lane group when the group's pending slots agree, else one per lane
template <int LPF>
__device__ __forceinline__ void flush_pending(const DecodeArgs& a, uint32_t sub, uint32_t pslot,
                                              unsigned long long pbest) {
  const uint32_t hi = pslot == 0xffffffffu ? 0u : pslot + 1;
  const uint32_t lo = pslot == 0xffffffffu ? 0xffffffffu : pslot + 1;
  const uint32_t mx = grp_reduce<LPF>(hi, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
  const uint32_t mn = grp_reduce<LPF>(lo, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
  const unsigned long long b = grp_max64<LPF>(pslot == 0xffffffffu ? 0ull : pbest);
  if (mx != 0 && mn == mx) {
    if (sub == 0) batch_max(&a.batch[mx - 1], b);
  } else if (pslot != 0xffffffffu) {
    batch_max(&a.batch[pslot], pbest);
  }
}

// Steps 5-6 of the fused kernels for the file of this lane group whose plaintext sits in LDS at
// fl: VersionBytes data-version check (crdt-enc/src/lib.rs:504-505), rmp-serde Vec<Dot<Uuid>>
// decode (lib.rs:507) and the max-fold of the dots of applied files (VClock::apply).  `live` =
// the file is active and its tag verified.  Called from wave-uniform control flow (ballots).
// the supported data versions (Core's supported_data_versions), the first two held in registers
// for the whole kernel so the per-file check issues no global load
struct SupVers {
  uint4 v0, v1;
  __device__ __forceinline__ explicit SupVers(const DecodeArgs& a) {
    v0 = a.n_supported > 0 ? *reinterpret_cast<const uint4*>(a.supported) : make_uint4(0, 0, 0, 0);
    v1 = a.n_supported > 1 ? *reinterpret_cast<const uint4*>(a.supported + 16) : make_uint4(0, 0, 0, 0);
  }
  __device__ __forceinline__ bool has(const DecodeArgs& a, const uint4& dv) const {
    // whole-vector compares without short circuits: one LDS read of dv and four word ops (word
    // by word, each compare was its own LDS read behind a branch).  v_bitop3 (a ^ b) | c keeps
    // the compiler from turning the OR of XORs back into four compares.
    auto eq = [&](const uint4& x) {
      uint32_t d = dv.x ^ x.x;
      d = __builtin_amdgcn_bitop3_b32(dv.y, x.y, d, 0xbe);
      d = __builtin_amdgcn_bitop3_b32(dv.z, x.z, d, 0xbe);
      d = __builtin_amdgcn_bitop3_b32(dv.w, x.w, d, 0xbe);
      return d == 0;
    };
    bool found = ((uint32_t)(a.n_supported > 0) & (uint32_t)eq(v0)) | ((uint32_t)(a.n_supported > 1) & (uint32_t)eq(v1));
    for (uint32_t s = 2; s < a.n_supported; s++) found |= eq(*reinterpret_cast<const uint4*>(a.supported + 16 * s));
    return found;
  }
};

// `prefetch` (the next file's parameters) is called once, after the decode's first round: a
// global load issued before the round's actor-table lookups would be waited for with them
// (vmcnt counts in order), exposing its latency.
// PN: the op grammar is Vec<pncounter::Op<Uuid>> (canon_pn_op / parse_pn_op) and a.batch holds two
// planes, Pos at [slot] and Neg at [slot + mask + 1]; the fold index carries the plane, so the
// pending (index, max), its carry and the flush are the Dot form's.  Every PN difference is an
// `if constexpr`: the Dot instantiations compile the code they always did.
template <int LPF, bool CARRY = false, bool PN = false, typename Pf>
__device__ __forceinline__ void decode_fold(const DecodeArgs& a, const SupVers& sup, const uint8_t* fl,
                                            uint32_t len, bool live, bool apply, uint32_t f,
                                            uint32_t grp, uint32_t sub, DecState& S, Pf&& prefetch) {
  int32_t st = CE_OK;
  if (live) {
    if (len < 16) st = CE_ERR_PT_LEN;
    else if (!sup.has(a, *reinterpret_cast<const uint4*>(fl))) st = CE_ERR_PT_VERSION;
  }
  bool pf_done = false;
  const uint8_t* body = fl + 16;
  const uint32_t blen = len >= 16 ? len - 16 : 0;
  uint64_t remaining = 0;
  uint32_t pos = 0;
  if (live && st == CE_OK) {
    Rd r{body, blen, 0};
    uint64_t count = 0;
    if (!rd_array_hdr(r, &count) || count > blen) st = CE_ERR_DECODE;
    else { remaining = count; pos = (uint32_t)r.i; }
  }
  const bool do_fold = live && st == CE_OK && apply;
  // pending max per lane: flushed with atomicMax when the lane's actor changes (CARRY: from
  // the previous file on, and the caller flushes after its last file)
  uint32_t pslot = CARRY ? S.pslot : 0xffffffffu;
  unsigned long long pbest = CARRY ? S.pbest : 0ull;
  auto fold_slot = [&](uint32_t slot, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3,
                       unsigned long long ctr) {
    if (slot == 0xffffffffu) {
      const uint32_t mi = atomicAdd(&a.counters[4], 1u);
      if (mi < a.miss_cap) a.miss_list[mi] = make_uint4(k0, k1, k2, k3);
      a.refold[f] = 1;
    } else if (slot == pslot) {
      pbest = ctr > pbest ? ctr : pbest;
    } else {
      if (pslot != 0xffffffffu) batch_max(&a.batch[pslot], pbest);
      pslot = slot;
      pbest = ctr;
    }
  };
  // per-lane cache of the last resolved actor: a file's dots are usually its writer's
  auto cached = [&](uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {
    return k0 == S.ck0 && k1 == S.ck1 && k2 == S.ck2 && k3 == S.ck3 && S.cslot != 0xffffffffu;
  };
  auto remember = [&](uint32_t slot, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {
    if (slot != 0xffffffffu) { S.ck0 = k0; S.ck1 = k1; S.ck2 = k2; S.ck3 = k3; S.cslot = slot; }
  };
  auto fold_dot = [&](uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3, unsigned long long ctr,
                      uint32_t dir = 0) {
    uint32_t slot;
    if (cached(k0, k1, k2, k3)) slot = S.cslot;
    else {
      slot = lookup_slot1(a.table, a.mask, a.nil_actor, k0, k1, k2, k3);
      remember(slot, k0, k1, k2, k3);
    }
    if constexpr (PN) {  // the direction selects the plane (the cache keeps the plain slot)
      if (slot != 0xffffffffu) slot += dir * (a.mask + 1u);
    }
    fold_slot(slot, k0, k1, k2, k3, ctr);
  };
  // Template path (a writer's own increments, the common GCounter op file): Dot 0 canonical and
  // every Dot carrying Dot 0's 34-byte prefix -- the same actor and marker, hence the same
  // length L0 > 34 and a canonical Dot -- checked as whole-word compares against Dot 0; each
  // lane keeps the max counter of its Dots.  Nothing is folded unless every Dot of the file
  // verifies: any other file (a Dot of another actor, a non-canonical Dot, fixint counters)
  // goes on to the paths below from Dot 0, exactly as if this block were absent.  Mixed-actor
  // files stop after their first LPF Dots.  Folding the max counter of Dots that all name one
  // actor is what folding them one by one does (VClock::apply, crdt-enc/src/lib.rs:533-535).
  // (Not built for PN: it would need one max per direction.)
  if constexpr (!PN) {
    uint32_t L0 = 0;
    if (live && st == CE_OK && remaining > 1 && pos + 34 <= blen) L0 = dot_len_of_marker(body[pos + 33]);
    bool tp = L0 > 34u && (uint64_t)pos + remaining * L0 <= blen;
    if (__any(tp)) {
      const uint32_t* b32 = reinterpret_cast<const uint32_t*>(body);
      uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      if (tp) {
        // Dot 1's actor bytes against Dot 0's first: files whose Dots name many actors (C2
        // variant B) leave before Dot 0's full check
        const uint32_t p0 = pos + 9u, p1 = pos + L0 + 9u;
        const uint32_t* d0 = b32 + (p0 >> 2);
        const uint32_t* d1 = b32 + (p1 >> 2);
        uint32_t e0[5], e1[5];
#pragma unroll
        for (int q = 0; q < 5; q++) {
          e0[q] = d0[q];
          e1[q] = d1[q];
        }
        uint32_t diff = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
          diff |= __builtin_amdgcn_alignbyte(e0[q + 1], e0[q], p0) ^ __builtin_amdgcn_alignbyte(e1[q + 1], e1[q], p1);
        tp = diff == 0;
      }
      if (__any(tp)) {
        // Dot 0 in full (its actor is the file's).  The window is read by every lane of the wave
        // -- a lane off the template path reads its own region at pos, a few bytes in, and its
        // result is dropped -- so the words stay in registers for the per-lane layout below
        // instead of being read from LDS and aligned a second time.
        uint32_t w[12];
        {
          const uint32_t* d = b32 + (pos >> 2);
          uint32_t dd[13];
#pragma unroll
          for (int q = 0; q < 13; q++) dd[q] = d[q];
#pragma unroll
          for (int q = 0; q < 12; q++) w[q] = __builtin_amdgcn_alignbyte(dd[q + 1], dd[q], pos);
        }
        unsigned long long c0;
        tp = ((uint32_t)tp & (uint32_t)canon_dot(w, L0, a0, a1, a2, a3, c0)) != 0;
        if (__any(tp)) {
          // this lane's Dots k = sub + LPF j all start at byte shift s (LPF L0 = 0 mod 4): Dot 0's
          // prefix laid out at that shift, E[q] = bytes 4q - s .. 4q - s + 3 of Dot 0, with the bytes
          // outside the prefix masked in the first and last words (M0, M8, M9).  E[q] is bytes
          // 4 - s .. 7 - s of the pair (w[q - 1], w[q]): one v_perm each, its selector per lane.
          // (E[0]'s bytes before Dot 0 and E[9]'s past w[8] are masked, so zeros stand in there.)
          const uint32_t s = (pos + sub * L0) & 3u;
          const uint32_t esel = 0x07060504u - 0x01010101u * s;
          uint32_t E[10];
#pragma unroll
          for (int q = 0; q < 10; q++)
            E[q] = __builtin_amdgcn_perm(q < 9 ? w[q] : 0u, q > 0 ? w[q - 1] : 0u, esel);
          // the next file's parameters: issued once the template path is taken and Dot 0's window
          // is consumed (it lands under the checks below; the per-Dot path issues it after its
          // first round, whose actor-table loads would otherwise wait for it -- vmcnt counts in
          // order)
          prefetch();
          pf_done = true;
          const uint32_t M0 = ~0u << (8u * s);
          const uint32_t M8 = s >= 2 ? ~0u : (s == 1 ? 0xffffffu : 0xffffu);
          const uint32_t M9 = s == 3 ? 0xffu : 0u;
          const uint32_t cw = L0 - 34u;                       // counter bytes: 1, 2, 4 or 8
          const uint32_t csh = cw < 4 ? 32u - 8u * cw : 0u;
          const uint32_t cnt = tp ? (uint32_t)remaining : 0u;
          uint32_t lim = cnt;  // the loop's bound: 0 once the group is off the path, so that "in"
                               // is one compare (a vote on tp && k < cnt costs two more per trip)
          // the counter's first four bytes sit at byte s + 2 of the words D[8..10] (34 = 32 + 2):
          // big-endian bytes s .. s + 3 of D[8..10] >> 16, reversed by the same v_perm
          const uint32_t csel = 0x00010203u + 0x01010101u * s;
          uint32_t bad = 0, mx = 0;
          unsigned long long mx64 = 0;
          for (uint32_t j = 0;; j++) {
            const uint32_t k = sub + LPF * j;
            const bool in = k < lim;
            if (!__any(in)) break;
            if (in) {
              const uint32_t c = pos + k * L0;
              const uint32_t* D = b32 + (c >> 2);
              // bad |= (D ^ E) [& M] over the ten words, as two chains of (D ^ E) | x
              uint32_t x = __builtin_amdgcn_bitop3_b32(D[0], E[0], M0, 0x28);  // (D ^ E) & M
              uint32_t y = __builtin_amdgcn_bitop3_b32(D[8], E[8], M8, 0x28);
              const uint32_t z = __builtin_amdgcn_bitop3_b32(D[9], E[9], M9, 0x28);
              x = __builtin_amdgcn_bitop3_b32(D[1], E[1], x, 0xbe);  // (D ^ E) | x
              y = __builtin_amdgcn_bitop3_b32(D[2], E[2], y, 0xbe);
              x = __builtin_amdgcn_bitop3_b32(D[3], E[3], x, 0xbe);
              y = __builtin_amdgcn_bitop3_b32(D[4], E[4], y, 0xbe);
              x = __builtin_amdgcn_bitop3_b32(D[5], E[5], x, 0xbe);
              y = __builtin_amdgcn_bitop3_b32(D[6], E[6], y, 0xbe);
              x = __builtin_amdgcn_bitop3_b32(D[7], E[7], x, 0xbe);
              bad |= x | y | z;
              const uint32_t c89 = __builtin_amdgcn_alignbyte(D[9], D[8], 2);
              const uint32_t c9a = __builtin_amdgcn_alignbyte(D[10], D[9], 2);
              const uint32_t hi = __builtin_amdgcn_perm(c9a, c89, csel);
              if (cw == 8) {
                const uint32_t u = c + 34u;  // counter bytes at shift (c + 34) mod 4
                const uint32_t* Cc = b32 + (u >> 2);
                const uint32_t lo = bswap32(__builtin_amdgcn_alignbyte(Cc[2], Cc[1], u));
                const unsigned long long v = ((unsigned long long)hi << 32) | lo;
                mx64 = v > mx64 ? v : mx64;
              } else {
                const uint32_t v = hi >> csh;
                mx = v > mx ? v : mx;
              }
            }
            if (j == 0 && grp_bits<LPF>(bad != 0, grp)) {  // another actor: stop early
              tp = false;
              lim = 0;
            }
          }
          if (grp_bits<LPF>(bad != 0, grp)) tp = false;
          if (tp) {
            if (do_fold && sub < cnt) fold_dot(a0, a1, a2, a3, cw == 8 ? mx64 : (unsigned long long)mx);
            remaining = 0;
          }
        }
      }
    }
  }
  // fast path: every Dot canonical with the first Dot's length L0, so Dot i sits at pos + i L0.
  // A round takes two Dots per lane (done + sub and done + LPF + sub): their 26 LDS reads are in
  // flight together.  It stops at the first Dot that is not canonical with length L0 (nothing
  // past it is folded); the sequential loop below takes over from there.
  if constexpr (PN) {
    // the same rounds over canonical Ops: two per lane at the first Op's length, 15 aligned LDS
    // dwords each -> the 56-byte window at the Op's byte shift
    uint32_t L0 = 0;
    if (live && st == CE_OK && remaining > 0 && pos + 39 <= blen) L0 = pn_len_of_marker(body[pos + 38]);
    uint32_t done = 0;
    bool fast = L0 != 0;
    for (;;) {
      const bool fb = fast && done < remaining;
      if (!__any(fb)) break;
      bool need[2], rd[2], valid[2];
      uint32_t k0[2], k1[2], k2[2], k3[2], cand[2], dir[2];
      unsigned long long ctr[2];
      uint32_t dd[2][15];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t i = done + sub + LPF * h;
        cand[h] = pos + i * L0;
        need[h] = fb && i < remaining;
        rd[h] = need[h] && cand[h] + L0 <= blen;
        const uint32_t* d = reinterpret_cast<const uint32_t*>(body) + ((rd[h] ? cand[h] : 0u) >> 2);
#pragma unroll
        for (int q = 0; q < 15; q++) dd[h][q] = d[q];
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t sh = cand[h] & 3;
        uint32_t w[14];
#pragma unroll
        for (int q = 0; q < 14; q++) w[q] = __builtin_amdgcn_alignbyte(dd[h][q + 1], dd[h][q], sh);
        valid[h] = canon_pn_op(w, L0, k0[h], k1[h], k2[h], k3[h], ctr[h], dir[h]) && rd[h];
      }
      const unsigned long long bad0 = grp_bits<LPF>(need[0] && !valid[0], grp);
      const unsigned long long bad1 = grp_bits<LPF>(need[1] && !valid[1], grp);
      const uint32_t kk = bad0 ? (uint32_t)__builtin_ctzll(bad0)
                               : bad1 ? (uint32_t)LPF + (uint32_t)__builtin_ctzll(bad1) : 2u * LPF;
      if (do_fold && need[0] && sub < kk) fold_dot(k0[0], k1[0], k2[0], k3[0], ctr[0], dir[0]);
      if (do_fold && need[1] && LPF + sub < kk) fold_dot(k0[1], k1[1], k2[1], k3[1], ctr[1], dir[1]);
      if (!pf_done) {
        prefetch();
        pf_done = true;
      }
      if (fb) {
        const bool bad = (bad0 | bad1) != 0;
        const uint64_t left = remaining - done;
        done += bad ? kk : (uint32_t)(left < 2u * LPF ? left : 2u * LPF);
        if (bad) fast = false;
      }
    }
    pos += done * L0;
    remaining -= done;
  } else {
    uint32_t L0 = 0;
    if (live && st == CE_OK && remaining > 0 && pos + 34 <= blen) L0 = dot_len_of_marker(body[pos + 33]);
    uint32_t done = 0;
    bool fast = L0 != 0;
    for (;;) {
      const bool fb = fast && done < remaining;
      if (!__any(fb)) break;
      bool need[2], rd[2], valid[2];
      uint32_t k0[2], k1[2], k2[2], k3[2], cand[2];
      unsigned long long ctr[2];
      uint32_t dd[2][13];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t i = done + sub + LPF * h;
        cand[h] = pos + i * L0;
        need[h] = fb && i < remaining;
        rd[h] = need[h] && cand[h] + L0 <= blen;
        const uint32_t* d = reinterpret_cast<const uint32_t*>(body) + ((rd[h] ? cand[h] : 0u) >> 2);
#pragma unroll
        for (int q = 0; q < 13; q++) dd[h][q] = d[q];
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t sh = cand[h] & 3;
        uint32_t w[12];
#pragma unroll
        for (int q = 0; q < 12; q++) w[q] = __builtin_amdgcn_alignbyte(dd[h][q + 1], dd[h][q], sh);
        valid[h] = canon_dot(w, L0, k0[h], k1[h], k2[h], k3[h], ctr[h]) && rd[h];
      }
      const unsigned long long bad0 = grp_bits<LPF>(need[0] && !valid[0], grp);
      const unsigned long long bad1 = grp_bits<LPF>(need[1] && !valid[1], grp);
      // valid prefix of the round's 2 LPF Dots (lane order within h, h = 0 first)
      const uint32_t kk = bad0 ? (uint32_t)__builtin_ctzll(bad0)
                               : bad1 ? (uint32_t)LPF + (uint32_t)__builtin_ctzll(bad1) : 2u * LPF;
      if (do_fold && need[0] && sub < kk) fold_dot(k0[0], k1[0], k2[0], k3[0], ctr[0]);
      if (do_fold && need[1] && LPF + sub < kk) fold_dot(k0[1], k1[1], k2[1], k3[1], ctr[1]);
      if (!pf_done) {
        prefetch();
        pf_done = true;
      }
      if (fb) {
        const bool bad = (bad0 | bad1) != 0;
        const uint64_t left = remaining - done;
        done += bad ? kk : (uint32_t)(left < 2u * LPF ? left : 2u * LPF);
        if (bad) fast = false;
      }
    }
    pos += done * L0;
    remaining -= done;
  }
  if (!pf_done) {
    prefetch();
    pf_done = true;
  }
  for (;;) {
    const bool busy = live && st == CE_OK && remaining > 0;
    if (!__any(busy)) break;
    // round: lane sub reads the candidate Dot at pos + sub * Ls.  Lane 0 is at a Dot start
    // whatever Ls is and checks its Dot at its own marker's length; lanes >= 1 are at Dot
    // starts only when every earlier Dot of the round had length Ls.
    bool valid = false;
    uint32_t Lme = 0;
    uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0, dir = 0;
    unsigned long long ctr = 0;
    const uint32_t cand = pos + sub * S.Ls;
    if constexpr (PN) {
      if (busy && sub < remaining && cand + 47 <= blen) {
        const uint32_t* d = reinterpret_cast<const uint32_t*>(body) + (cand >> 2);
        const uint32_t sh = cand & 3;
        uint32_t dd[15];
#pragma unroll
        for (int i = 0; i < 15; i++) dd[i] = d[i];
        uint32_t w[14];
#pragma unroll
        for (int i = 0; i < 14; i++) w[i] = __builtin_amdgcn_alignbyte(dd[i + 1], dd[i], sh);
        Lme = pn_len_of_marker((w[9] >> 16) & 0xff);
        const uint32_t L = sub == 0 ? Lme : S.Ls;
        valid = ((uint32_t)canon_pn_op(w, L, k0, k1, k2, k3, ctr, dir) & (uint32_t)(Lme != 0) &
                 (uint32_t)(cand + L <= blen)) != 0;
      }
    } else
    if (busy && sub < remaining && cand + 34 <= blen) {
      // 13 aligned LDS dwords -> the 48-byte window at cand
      const uint32_t* d = reinterpret_cast<const uint32_t*>(body) + (cand >> 2);
      const uint32_t sh = cand & 3;
      uint32_t dd[13];
#pragma unroll
      for (int i = 0; i < 13; i++) dd[i] = d[i];
      uint32_t w[12];
#pragma unroll
      for (int i = 0; i < 12; i++) w[i] = __builtin_amdgcn_alignbyte(dd[i + 1], dd[i], sh);
      Lme = dot_len_of_marker((w[8] >> 8) & 0xff);
      const uint32_t L = sub == 0 ? Lme : S.Ls;
      valid = ((uint32_t)canon_dot(w, L, k0, k1, k2, k3, ctr) & (uint32_t)(Lme != 0) &
               (uint32_t)(cand + L <= blen)) != 0;
    }
    constexpr unsigned long long GM = LPF == 64 ? ~0ull : ((1ull << LPF) - 1);
    const unsigned long long vb = grp_bits<LPF>(valid, grp);
    uint32_t k = vb == GM ? (uint32_t)LPF : (uint32_t)__builtin_ctzll(~vb);
    const bool m0 = grp_bits<LPF>(sub == 0 && Lme == S.Ls, grp) != 0;
    if (!m0 && k > 1) k = 1;  // lanes >= 1 read at the wrong offsets
    // next speculation: the first lane past the round sits exactly on the next Dot
    const uint32_t inf = m0 ? k : 0u;
    const uint32_t code = sub == inf ? len_code(PN ? Lme - kPnOpExtra : Lme) : 0u;
    const uint32_t nc = (grp_bits<LPF>(code & 1, grp) ? 1u : 0u) |
                        (grp_bits<LPF>(code & 2, grp) ? 2u : 0u) |
                        (grp_bits<LPF>(code & 4, grp) ? 4u : 0u);
    const uint32_t Lold = S.Ls;
    if (nc) S.Ls = code_len(nc) + (PN ? kPnOpExtra : 0u);  // when !m0 this is lane 0's own length
    // general grammar for one element (group leader), e.g. reordered keys / array form
    const bool general = busy && k == 0;
    bool fold_me = do_fold && busy && sub < k;
    if (__any(general)) {
      int gok = 0;
      uint32_t npos = pos;
      if (general && sub == 0) {
        Rd q{body, blen, pos};
        uint64_t aoff = 0, c = 0;
        if constexpr (PN) gok = parse_pn_op(q, &aoff, &c, &dir);
        else gok = parse_dot(q, &aoff, &c);
        if (gok == 1) {
          k0 = ld_le32(body + aoff); k1 = ld_le32(body + aoff + 4);
          k2 = ld_le32(body + aoff + 8); k3 = ld_le32(body + aoff + 12);
          ctr = c;
          npos = (uint32_t)q.i;
          fold_me = do_fold;
        }
      }
      gok = __shfl(gok, (int)(grp * LPF));
      npos = __shfl(npos, (int)(grp * LPF));
      if (general) {
        if (gok != 1) st = CE_ERR_DECODE;
        else { pos = npos; remaining -= 1; }
      }
    }
    if (fold_me) fold_dot(k0, k1, k2, k3, ctr, dir);
    if (busy && k > 0) {
      pos += m0 ? k * Lold : S.Ls;  // !m0: k == 1 and Ls == lane 0's Dot length
      remaining -= k;
    }
  }
  // flush: one atomicMax per file when the group's pending actors agree
  if (CARRY) {
    S.pslot = pslot;
    S.pbest = pbest;
  } else {
    const uint32_t hi = pslot == 0xffffffffu ? 0u : pslot + 1;
    const uint32_t lo = pslot == 0xffffffffu ? 0xffffffffu : pslot + 1;
    const uint32_t mx = grp_reduce<LPF>(hi, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
    const uint32_t mn = grp_reduce<LPF>(lo, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
    const unsigned long long b = grp_max64<LPF>(pslot == 0xffffffffu ? 0ull : pbest);
    if (mx != 0 && mn == mx) {
      if (sub == 0) batch_max(&a.batch[mx - 1], b);
    } else if (pslot != 0xffffffffu) {
      batch_max(&a.batch[pslot], pbest);
    }
  }
  if (live && st != CE_OK && sub == 0) {
    a.status[f] = st;
    atomicAdd(&a.counters[3], 1u);
    atomicMin(&a.counters[5], f);
  }
}

template <int LPF>
__global__ __launch_bounds__(FusedCfg<LPF>::WPB * 64, FusedCfg<LPF>::WAVES_PER_SIMD)
void k_open_fold_small(DecodeArgs a) {
  using C = FusedCfg<LPF>;
  constexpr int F = C::F;
  constexpr int PPL = 256 / LPF;  // ciphertext pieces per lane (one page)
  __shared__ __attribute__((aligned(16))) uint8_t lds[C::WPB * F * kRegion];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wib = threadIdx.x >> 6;
  const uint32_t grp = lane / LPF, sub = lane % LPF;
  uint8_t* fl = lds + (wib * F + grp) * kRegion;
  const uint32_t ngroups = (a.n + F - 1) / F;
  const uint32_t stride = gridDim.x * C::WPB;

  uint32_t g = bcast(blockIdx.x * C::WPB + wib);
  FilePre nx = load_pre<C::LOG + C::LOGCH>(a, g * F + grp);
  const SupVers sup(a);
  // decode state carried across files: speculated Dot length, per-lane actor cache
  DecState S{38, 0, 0, 0, 0, 0xffffffffu};
  AuthFails fails;

  for (; g < ngroups; g += stride) {
    const uint32_t f = g * F + grp;
    const FilePre cur = nx;
    const uint32_t len = cur.ok && cur.len <= kSmallMax ? cur.len : 0u;
    const bool act = cur.ok && cur.len <= kSmallMax;
    const uint32_t nblk_ct = (len + 15) >> 4;
    // inactive lanes read 16 B of the (always allocated) params array instead of the blob
    const uint8_t* src = act ? a.blob + (((uint64_t)cur.in_hi << 32) | cur.in_off)
                             : reinterpret_cast<const uint8_t*>(a.params);
    const FileParams* Pp = a.params + (act ? f : 0);

    // 1) ciphertext pieces -> registers (issued first: latency hides under the ChaCha20).
    //    Poly1305 blocks are dealt from the END: lane sub, slot t holds block b = nblk_ct - sub -
    //    LPF t (b == nblk_ct: the length block; b < 0: none), whose weight is r^(sub + 1) *
    //    (r^LPF)^t -- every lane's Horner ends at weight 1 whatever the length (shorter files
    //    only drop leading terms).
    uint4 ct[PPL + 1];
#pragma unroll
    for (int j = 0; j <= PPL; j++) {
      const int32_t blk = (int32_t)nblk_ct - (int32_t)sub - LPF * j;
      const uint32_t boff = blk >= 0 && blk < (int32_t)nblk_ct ? (uint32_t)blk * 16u : 0u;
      // the 16-byte tag follows the ciphertext, so a 16-byte load at any boff < len stays
      // inside the file; bytes past len are zeroed below (Poly1305 pad16, plaintext tail).
      // Slots before the first piece load the file's first piece (in bounds), never used.
      ct[j] = *reinterpret_cast<const uint4*>(src + boff);
    }
    __builtin_amdgcn_wave_barrier();

    // 2) keystream: lane computes blocks sub + LPF*k (ChaCha20 counter 1 + block); the
    //    counter-independent first-round work is shared by the lane's F blocks
    const ChachaPre cpre = chacha_pre(cur.key, 0u, cur.n2a, cur.n2b);
#pragma unroll
    for (int k = 0; k < F; k++) {
      const uint32_t b = sub + LPF * k;
      if (act && b * 64 < len) {
        uint32_t kb[16];
        chacha_block_pre(cpre, cur.key, 1u + b, 0u, cur.n2a, cur.n2b, kb);
        uint4* kd = reinterpret_cast<uint4*>(fl + b * kKsStride);
        kd[0] = make_uint4(kb[0], kb[1], kb[2], kb[3]);
        kd[1] = make_uint4(kb[4], kb[5], kb[6], kb[7]);
        kd[2] = make_uint4(kb[8], kb[9], kb[10], kb[11]);
        kd[3] = make_uint4(kb[12], kb[13], kb[14], kb[15]);
      }
    }
    __builtin_amdgcn_wave_barrier();

    // tree powers r^(2^k), k < LOG + 2 (r^LPF, r^2LPF combine the chains), and s || expected
    // tag: 16-byte loads issued now, used after the Horner pass (their latency hides under it).
    // Inactive lanes read params[0].
    constexpr int NPOW = C::LOG + C::NCH - 1 < 7 ? C::LOG + C::NCH - 1 : 7;
    constexpr int NRW = 5 * NPOW;
    uint32_t rp[(NRW + 3) / 4 * 4];
#pragma unroll
    for (int q = 0; q < (NRW + 3) / 4; q++) {
      const uint4 v = *reinterpret_cast<const uint4*>(&Pp->rpow[0][0] + 4 * q);
      rp[4 * q] = v.x; rp[4 * q + 1] = v.y; rp[4 * q + 2] = v.z; rp[4 * q + 3] = v.w;
    }
    const uint4 sv4 = *reinterpret_cast<const uint4*>(Pp->s);
    const uint4 tg4 = *reinterpret_cast<const uint4*>(Pp->tag);

    // 3) XOR, plaintext into LDS (over consumed keystream), NCH Horner chains in r^64 over the
    //    lane's slots, highest slot first (slots before the first piece are leading zeros)
    L5 RS;
#pragma unroll
    for (int i = 0; i < 5; i++) RS.v[i] = cur.R[i];
    L5 acc[C::NCH];
#pragma unroll
    for (int c = 0; c < C::NCH; c++) acc[c] = L5{{0, 0, 0, 0, 0}};
#pragma unroll
    for (int j = PPL; j >= 0; j--) {
      const int32_t blk = (int32_t)nblk_ct - (int32_t)sub - LPF * j;
      const int c = j % C::NCH;
      if (act && blk == (int32_t)nblk_ct) {
        acc[c] = add5(mulmod(acc[c], RS), block_limbs(0u, 0u, len, 0u));  // le64(0) || le64(len)
      } else if (act && blk >= 0) {
        uint32_t kw_mask[4] = {~0u, ~0u, ~0u, ~0u};
        const uint32_t q = (uint32_t)blk;  // piece index within the page
        const uint4 k4 = *reinterpret_cast<const uint4*>(fl + (q >> 2) * kKsStride + (q & 3) * 16);
        uint4 x = ct[j];
        const uint32_t boff = q * 16;
        if (boff + 16 > len) {  // tail piece: zero the bytes past the ciphertext
          const uint32_t rem = len - boff;
          uint32_t xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const uint32_t lo = 4 * i;
            const uint32_t keep = rem >= lo + 4 ? 0xffffffffu
                                  : (rem <= lo ? 0u : ((1u << (8 * (rem - lo))) - 1));
            xw[i] &= keep;
            kw_mask[i] = keep;
          }
          x = make_uint4(xw[0], xw[1], xw[2], xw[3]);
        }
        uint4 y = make_uint4(x.x ^ (k4.x & kw_mask[0]), x.y ^ (k4.y & kw_mask[1]),
                             x.z ^ (k4.z & kw_mask[2]), x.w ^ (k4.w & kw_mask[3]));
        *reinterpret_cast<uint4*>(fl + boff) = y;
        acc[c] = add5(mulmod(acc[c], RS), block_limbs(x.x, x.y, x.z, x.w));
      }
    }
    // lane value = sum_c acc_c * (r^LPF)^c
    L5 lv = acc[0];
    {
      L5 p1, p2;
#pragma unroll
      for (int i = 0; i < 5; i++) {
        p1.v[i] = rp[5 * C::LOG + i];
        p2.v[i] = C::NCH > 2 ? rp[5 * (C::LOG + 1) + i] : 0u;
      }
      if (C::NCH > 1) lv = add5(lv, mulmod(acc[C::NCH > 1 ? 1 : 0], p1));
      if (C::NCH > 2) lv = add5(lv, mulmod(acc[C::NCH > 2 ? 2 : 0], p2));
      if (C::NCH > 3) lv = add5(lv, mulmod(acc[C::NCH > 3 ? 3 : 0], mulmod(p1, p2)));
      lv = carry5(lv);
    }
    __builtin_amdgcn_wave_barrier();

    // 4) cross-lane tree inside the group: U = sum_s lane_s * r^s (level k adds lane s + 2^k
    //    times r^(2^k): DPP row shifts up to 8 lanes), then T = U * r.  Only position 0 (sub 0)
    //    ends with the sum.
    L5 v = lv;
#pragma unroll
    for (int k = 0; k < C::LOG; k++) {
      L5 rk;
#pragma unroll
      for (int i = 0; i < 5; i++) rk.v[i] = rp[5 * k + i];
      L5 o;
#pragma unroll
      for (int i = 0; i < 5; i++)
        o.v[i] = k < 4 ? row_down(v.v[i], 1 << k) : (uint32_t)__shfl_down((int)v.v[i], 1u << k);
      v = carry5(add5(v, mulmod(o, rk)));
    }
    L5 r1;
#pragma unroll
    for (int i = 0; i < 5; i++) r1.v[i] = rp[i];
    const L5 tot = mulmod(v, r1);
    bool tag_ok = false;
    if (act && sub == 0) {
      const uint32_t sv[4] = {sv4.x, sv4.y, sv4.z, sv4.w};
      uint32_t tag[4];
      poly_tag(tot, sv, tag);
      tag_ok = ((tag[0] ^ tg4.x) | (tag[1] ^ tg4.y) | (tag[2] ^ tg4.z) | (tag[3] ^ tg4.w)) == 0;
      if (!tag_ok) a.status[f] = CE_ERR_AUTH;
    }
    fails.add(act && sub == 0 && !tag_ok, f);
    const bool ok = grp_bits<LPF>(tag_ok, grp) != 0;

    // 5)+6) data-version check, decode from LDS, fold;
    // the next iteration's parameters are loaded inside (their latency hides under the decode)
    decode_fold<LPF>(a, sup, fl, len, act && ok, cur.apply != 0, f, grp, sub, S,
                     [&] { nx = load_pre<C::LOG + C::LOGCH>(a, (g + stride) * F + grp); });
    __builtin_amdgcn_wave_barrier();
  }
  fails.flush(a);
}

// Resident blocks per CU for a kernel, from the occupancy calculator (LDS and VGPRs both
// bound it); the grid-stride loop then runs exactly one round of resident blocks.
template <typename K>
static uint32_t resident_blocks(K kernel, int threads) {
  int dev = 0, per_cu = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess ||
      per_cu < 1)
    per_cu = 1;
  return (uint32_t)(per_cu * cus);
}

hipError_t launch_open_fold_small(hipStream_t s, const DecodeArgs& a, int files_per_wave, OpenLaunchLog& log) {
  if (a.n == 0) return hipSuccess;
  static const uint32_t res16 = resident_blocks(k_open_fold_small<16>, 128);
  static const uint32_t res32 = resident_blocks(k_open_fold_small<32>, 256);
  static const uint32_t res64 = resident_blocks(k_open_fold_small<64>, 256);
  const uint32_t groups = (a.n + files_per_wave - 1) / files_per_wave;
  if (files_per_wave == 4) {
    const uint32_t blocks = log.grid(std::min<uint32_t>((groups + 1) / 2, res16), "open_small_lpf16");
    hipLaunchKernelGGL(k_open_fold_small<16>, dim3(blocks), dim3(128), 0, s, a);
  } else if (files_per_wave == 2) {
    const uint32_t blocks = log.grid(std::min<uint32_t>((groups + 3) / 4, res32), "open_small_lpf32");
    hipLaunchKernelGGL(k_open_fold_small<32>, dim3(blocks), dim3(256), 0, s, a);
  } else {
    const uint32_t blocks = log.grid(std::min<uint32_t>((groups + 3) / 4, res64), "open_small_lpf64");
    hipLaunchKernelGGL(k_open_fold_small<64>, dim3(blocks), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

// ----------------------------------------------------------------------------------------
// k_open_fold_v2<LPF>: the same open + decode + fold, with whole ChaCha20 blocks per lane.
//   Lane sub of a file's LPF-lane group owns blocks b = nblk - 1 - sub - LPF k (k < 64 / LPF,
//   only b >= 0), dealt from the END: lane 0 slot 0 always holds the last, possibly partial,
//   block.  The lane loads its blocks' 64-byte ciphertext runs, computes their keystream in
//   registers and writes only plaintext to LDS: 4 KiB per file and one LDS store per piece
//   (k_open_fold_small stores the keystream, reads it back transposed and stores plaintext:
//   5 KiB per file, three LDS operations per piece).  One wave per workgroup: 16 KiB of LDS
//   (LPF 16, 10 waves per CU) or 8 KiB (LPF 32, 20 waves per CU).
//   Poly1305 over the lane's blocks, earliest first: G = Horner in r over the block's pieces,
//   acc = acc r^(4 LPF) + G.  Lane s >= 1 ends at piece 4 nblk - 1 - 4 s.  Lane 0 keeps its last
//   block apart (G'), so its chain ends at piece 4 nblk - 1 - 4 LPF, where a lane LPF would.
//   Moving every chain one lane down puts them at tree positions q = 0..LPF-1 four pieces apart
//   (q = 0 latest): U = sum_q v_q r^(4q) through the DPP tree in r^4 .. r^(2 LPF).  With
//   delta = 4 nblk - npc (pieces missing from the last block), T = (U r^(5-delta) + G' r + lenblock) r.
// ----------------------------------------------------------------------------------------
static constexpr uint32_t kRegion2 = 4096;
// Regions of a wave's files start 4128 B apart (not 4096): the decode's LDS reads of two files
// in one 32-lane bank group then fall on different banks at equal offsets (4096 = 0 mod 32
// banks made every such pair collide; tools/lds_banks.py: 1.29 -> 1.0 extra cycles per read
// at the C2 Dot layout).  64 B of slack past the last region take the decode's over-reads.
static constexpr uint32_t kRegionStride2 = 4128;

template <int LPF>
struct V2Cfg {
  static constexpr int F = 64 / LPF;               // files per wave
  static constexpr int BPL = 64 / LPF;             // ChaCha20 blocks per lane (one page)
  static constexpr int LOG = LPF == 16 ? 4 : 5;    // tree levels
  static constexpr int NRP = LPF == 16 ? 8 : 9;    // 16-byte loads of r^(2^k), k <= LOG + 1
};

struct FilePre2 {
  uint32_t ok, apply, len, in_off, in_hi;
  uint32_t key[8];
  uint32_t n2a, n2b;
  uint32_t R1[5];   // r
  uint32_t R64[5];  // r^64
  // r^2: no kernel reads it from here (they load rpow[1] where they use it), yet dropping it is
  // not free: compiled without the member, every k_open_fold_v3 form and the 4-files-per-wave
  // k_open_fold_v2 come out 1 to 41 instructions shorter and k_open_fold_v3<false, false> one
  // VGPR larger (rpow[1] follows rpow[0], R1, in memory).  So it goes with a measured change,
  // not with a cleanup.
  uint32_t R2[5];
};

__device__ __forceinline__ FilePre2 load_pre2(const DecodeArgs& a, uint32_t f) {
  FilePre2 p;
  const bool in = f < a.n;
  const uint32_t fi = in ? f : 0u;
  const FileParams* Pp = a.params + fi;
  // status, only and apply are independent loads: no per-lane short circuit (that would wait
  // for each before issuing the next)
  const int32_t stv = a.status[fi];
  const uint32_t ov = a.only ? (uint32_t)a.only[fi] : 1u;
  const uint32_t av = a.apply ? (uint32_t)a.apply[fi] : 1u;
  p.ok = (uint32_t)in & (uint32_t)(stv == CE_OK) & (uint32_t)(ov != 0);
  p.apply = av != 0;
  p.len = Pp->len;
  p.in_off = (uint32_t)Pp->in_off;
  p.in_hi = (uint32_t)(Pp->in_off >> 32);
#pragma unroll
  for (int i = 0; i < 8; i++) p.key[i] = Pp->subkey[i];
  p.n2a = Pp->n2[0];
  p.n2b = Pp->n2[1];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    p.R1[i] = Pp->rpow[0][i];
    p.R64[i] = Pp->rpow[6][i];
    p.R2[i] = Pp->rpow[1][i];
  }
  return p;
}

// ---- Orswot op files decoded in the open (k_open_fold_v2's DS form) ------------------------
// C3's op files (~2 KiB of plaintext, 32 ops) used to go open -> plaintext in HBM -> a lane-per-
// file count pass -> scan -> a lane-per-file emit, reading the plaintext twice.  In the DS form a
// file of at most kDsFuseRegion bytes keeps its plaintext in LDS after the open and its 16 lanes
// decode it there (read_remote_ops' from_slice, crdt-enc/src/lib.rs:507, of a Vec<orswot::Op>):
//   1. the supported data version (lib.rs:504-505) and the Vec header (fixarray / array16 / 32);
//   2. candidate op starts: every byte position whose word is Add's or Rm's first four bytes
//      (81 a3 "Ad" / 81 a2 "Rm"), lane sub scanning dwords sub, sub + 16, ... (in order);
//   3. a lane per candidate proves the canonical form ce_dotset.hip's fast_orswot_op accepts
//      (one member; a one-entry clock; any uint width), resolves its actor (a one-entry cache,
//      then the table), and writes its row: op k of file f at col[f * rows + k];
//   4. the proven ops must be exactly the Vec's elements: as many as the header says, the first
//      where the header ends, each starting where the previous one ends.  A spurious proven
//      candidate inside an op, an op of another form, an unknown actor, a count past the rows,
//      any of it: the file's plaintext goes to HBM and the lane-per-file decode takes it
//      (done[f] = 0), so every file gets exactly the reference grammar's result.
// The offsets columns (add_mbeg, rm_cbeg, rm_mbeg) are not written: with one member / one clock
// entry per op they are the op's index plus the file's base (k_ds_untile adds it).
static constexpr uint32_t kDsStride = kDsFuseRegion + 96;  // plaintext + the windows' over-reads
static constexpr uint32_t kDsCandCap = 96;                  // candidate op starts per file
static constexpr uint32_t kDsVCap = 64;                     // proven ops per file (>= 47 B each)
static constexpr uint32_t kDsAuxHalves = kDsCandCap + 2 * kDsVCap;  // u16: cand, vpos, vlen
static constexpr uint32_t kAddMagic = 0x6441a381u;  // 81 a3 'A' 'd'
static constexpr uint32_t kRmMagic = 0x6d52a281u;   // 81 a2 'R' 'm'

// N LE words at byte x of a dword-aligned LDS region L (any alignment of x): N + 1 aligned dword
// reads shifted into place (indexed from L, so they stay LDS reads, not flat ones)
template <int N>
struct LdsWin {
  uint32_t w[N];
  __device__ __forceinline__ LdsWin(const uint32_t* L, uint32_t x) {
    const uint32_t* b = L + (x >> 2);
    const uint32_t sh = x & 3u;
    uint32_t d[N + 1];
#pragma unroll
    for (int k = 0; k <= N; k++) d[k] = b[k];
#pragma unroll
    for (int k = 0; k < N; k++) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  }
  __device__ __forceinline__ uint32_t word(int b) const {  // bytes [b, b + 4), b compile-time
    return (b & 3) ? __builtin_amdgcn_alignbyte(w[(b >> 2) + 1], w[b >> 2], b & 3) : w[b >> 2];
  }
  __device__ __forceinline__ uint32_t byte(int b) const { return (w[b >> 2] >> (8 * (b & 3))) & 0xffu; }
  // msgpack uint at byte b (positive fixint, cc, cd, ce, cf); *len = its size, 0 for another form
  __device__ __forceinline__ unsigned long long uint_at(int b, uint32_t* len) const {
    const uint32_t m = byte(b);
    const uint32_t x0 = __builtin_bswap32(word(b + 1)), x1 = __builtin_bswap32(word(b + 5));
    *len = m < 0x80u ? 1u : m == 0xccu ? 2u : m == 0xcdu ? 3u : m == 0xceu ? 5u : m == 0xcfu ? 9u : 0u;
    return m < 0x80u ? m : m == 0xccu ? x0 >> 24 : m == 0xcdu ? x0 >> 16 : m == 0xceu ? x0
                                                       : ((unsigned long long)x0 << 32) | x1;
  }
};

struct DsOp {
  uint32_t kind;  // 1 Add, 2 Rm, 0 not proven
  uint32_t len, u0, u1, u2, u3;
  unsigned long long ctr, mem;
};

// the op at byte x of a file's plaintext in LDS (len bytes), in the forms rmp-serde's
// to_vec_named writes for a one-member Add / a one-entry-clock Rm:
//   Add: 81 a3"Add" 82 a3"dot" 82 a5"actor" c4 10 <uuid> a7"counter" <uint> a7"members" 91 <uint>
//   Rm:  81 a2"Rm" 82 a5"clock" 81 a4"dots" 81 c4 10 <uuid> <uint> a7"members" 91 <uint>
__device__ __forceinline__ DsOp ds_parse_fast(const uint32_t* L, uint32_t x, uint32_t len) {
  DsOp o{};
  const LdsWin<13> v(L, x);  // bytes x .. x + 51
  uint32_t l = 0, y = 0;
  if (v.w[0] == kAddMagic && v.w[1] == 0x64a38264u && v.w[2] == 0xa582746fu && v.w[3] == 0x6f746361u &&
      (v.w[4] & 0xffffffu) == 0x10c472u && v.word(35) == 0x756f63a7u && v.word(39) == 0x7265746eu) {
    o.ctr = v.uint_at(43, &l);
    o.u0 = v.word(19); o.u1 = v.word(23); o.u2 = v.word(27); o.u3 = v.word(31);
    y = 43 + l;
    o.kind = l ? 1u : 0u;
  } else if (v.w[0] == kRmMagic && v.w[1] == 0x6c63a582u && v.w[2] == 0x816b636fu && v.w[3] == 0x746f64a4u &&
             v.w[4] == 0x10c48173u) {
    o.ctr = v.uint_at(36, &l);
    o.u0 = v.w[5]; o.u1 = v.w[6]; o.u2 = v.w[7]; o.u3 = v.w[8];
    y = 36 + l;
    o.kind = l ? 2u : 0u;
  }
  if (o.kind) {
    const LdsWin<5> m(L, x + y);  // "a7 members 91" <uint>: bytes y .. y + 19
    uint32_t lm = 0;
    if (m.word(0) == 0x6d656da7u && m.word(4) == 0x73726562u && m.byte(8) == 0x91u) o.mem = m.uint_at(9, &lm);
    o.len = y + 9 + lm;
    if (!lm || x + o.len > len) o.kind = 0;
  }
  return o;
}

// the dot-set actor id (ActorSlot.pad[0]) of a UUID through a one-entry per-lane cache
struct DsActorCache {
  uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0, id = 0xffffffffu;
  uint4 pk = make_uint4(0, 0, 0, 0);  // prime: the first probe's slot of the first op's UUID
  uint32_t pused = 0, pid = 0xffffffffu;
  // the first op's UUID (bytes 19.. of an Add, 20.. of an Rm at p0) and its first table probe,
  // loaded but not waited for; get() takes it when the slot holds that UUID
  __device__ __forceinline__ void prime(const DecodeArgs& a, const uint32_t* L, uint32_t p0, uint32_t len) {
    if (p0 + 40 > len) return;
    const LdsWin<6> w(L, p0);
    const uint32_t u = w.byte(1) == 0xa3u ? 19u : 20u;
    const LdsWin<4> v(L, p0 + u);
    k0 = v.w[0]; k1 = v.w[1]; k2 = v.w[2]; k3 = v.w[3];
    const ActorSlot& sl = a.table[actor_hash(k0, k1, k2, k3) & a.mask];
    pk = *reinterpret_cast<const uint4*>(sl.k);
    pused = sl.used;
    pid = sl.pad[0];
  }
  __device__ __forceinline__ uint32_t get(const DecodeArgs& a, const DsOp& o) {
    if (pused && o.u0 == k0 && o.u1 == k1 && o.u2 == k2 && o.u3 == k3 && pk.x == k0 && pk.y == k1 && pk.z == k2 &&
        pk.w == k3) {
      pused = 0;
      id = pid;
    }
    if (id != 0xffffffffu && o.u0 == k0 && o.u1 == k1 && o.u2 == k2 && o.u3 == k3) return id;
    const uint32_t h = lookup_slot(a.table, a.mask, o.u0, o.u1, o.u2, o.u3);
    if (h == 0xffffffffu) return h;
    k0 = o.u0; k1 = o.u1; k2 = o.u2; k3 = o.u3;
    id = a.table[h].pad[0];
    return id;
  }
};

// steps 1-4 above for the file of this lane group (act: its tag verified and its plaintext is
// in LDS at fl); returns whether the file was decoded (group-uniform).  Wave-uniform control flow.
template <int LPF>
__device__ __forceinline__ bool ds_fused_decode(const DecodeArgs& a, const SupVers& sup, const uint8_t* fl,
                                                uint16_t* aux, uint32_t len, bool act, uint32_t f, uint32_t grp,
                                                uint32_t sub) {
  DsActorCache cache;  // per file (a file's ops are mostly its writer's)
  static_assert(LPF <= 32, "group ballots are taken as 32-bit masks");
  const DsFuse& x = a.ds;
  const uint32_t* L = reinterpret_cast<const uint32_t*>(fl);
  const uint32_t lt = (1u << sub) - 1u;
  auto gb = [&](bool p) { return (uint32_t)grp_bits<LPF>(p, grp); };
  __syncthreads();  // the open's plaintext stores (one wave per workgroup)
  // 1) data version and Vec header
  bool ok = act && len >= 17;
  uint32_t cnt = 0, p0 = 0;
  if (ok) {
    const uint4 dv = *reinterpret_cast<const uint4*>(fl);
    const uint32_t w4 = L[4], w5 = L[5];
    const uint32_t h = w4 & 0xffu;
    ok = sup.has(a, dv);
    if ((h & 0xf0u) == 0x90u) {
      cnt = h & 15u;
      p0 = 17;
    } else if (h == 0xdcu) {
      cnt = (((w4 >> 8) & 0xffu) << 8) | ((w4 >> 16) & 0xffu);
      p0 = 19;
    } else if (h == 0xddu) {
      cnt = __builtin_bswap32(__builtin_amdgcn_alignbyte(w5, w4, 1));
      p0 = 21;
    } else {
      ok = false;
    }
    ok = ok && p0 <= len && cnt <= kDsVCap;
  }
  // the first op's actor (the file's writer, usually every op's): its first table probe issued now,
  // so the load lands during the scan (DsActorCache::prime)
  if (ok) cache.prime(a, L, p0, len);
  // 2) candidate op starts, in position order: positions whose bytes are 81 a2 / 81 a3 (an Add's or
  //    Rm's first two bytes; the proof in step 3 checks the rest).  Branch-free SWAR over two dwords
  //    per lane per round: g's byte j is zero iff byte j == 0x81 and byte j + 1 is a2 / a3, found
  //    exactly (no borrow between bytes); a dword holds at most two such positions (a member's
  //    last bytes can spell 81 a2 just before the next op).  Positions before p0 or past len are
  //    left to step 3 and the chain check (nothing there proves, or the chain fails and the lane
  //    decode takes the file).
  uint16_t* cand = aux;
  uint32_t nc = 0;
  const uint32_t dbeg = p0 >> 2, dend = (len + 3) >> 2;
  auto zbytes = [](uint32_t A, uint32_t B) {  // bit 8j + 7: bytes (j, j + 1) = 81, a2|a3
    const uint32_t g = (A ^ 0x81818181u) | ((__builtin_amdgcn_alignbyte(B, A, 1) ^ 0xa2a2a2a2u) & 0xfefefefeu);
    return ~(((g & 0x7f7f7f7fu) + 0x7f7f7f7fu) | g) & 0x80808080u;
  };
  for (uint32_t r = 0; __any(ok && dbeg + r < dend); r += 2 * LPF) {
    const uint32_t d = dbeg + r + 2 * sub;
    unsigned long long m = 0;
    if (ok && d < dend) {
      const uint32_t A = L[d], B = L[d + 1], Cw = L[d + 2];
      m = ((unsigned long long)zbytes(B, Cw) << 32) | zbytes(A, B);
    }
    // this lane's candidates (0..4) go after every lower lane's: a group prefix sum by bit planes
    const uint32_t c = (uint32_t)__popcll(m);
    const uint32_t b0 = gb(c & 1u), b1 = gb(c & 2u), b2 = gb(c & 4u);
    uint32_t idx = nc + __popc(b0 & lt) + 2 * __popc(b1 & lt) + 4 * __popc(b2 & lt);
    while (m) {
      if (idx < kDsCandCap) cand[idx] = (uint16_t)(4 * d + ((uint32_t)__builtin_ctzll(m) >> 3));
      idx++;
      m &= m - 1;
    }
    nc += __popc(b0) + 2 * __popc(b1) + 4 * __popc(b2);
  }
  ok = ok && nc <= kDsCandCap;
  __syncthreads();
  // 3) prove the candidates, rank the proven ones, write their rows
  uint16_t* vpos = aux + kDsCandCap;
  uint16_t* vlen = vpos + kDsVCap;
  uint32_t nv = 0, na = 0, nr = 0;
  bool miss = false;
  const size_t row0 = (size_t)f * x.rows;
  for (uint32_t r = 0; __any(ok && r < nc); r += LPF) {
    const uint32_t i = r + sub;
    DsOp o{};
    uint32_t pos = 0;
    if (ok && i < nc) {
      pos = cand[i];
      o = ds_parse_fast(L, pos, len);
    }
    const bool v = o.kind != 0;
    const uint32_t vb = gb(v), ab = gb(o.kind == 1), rb = gb(o.kind == 2);
    const uint32_t k = nv + __popc(vb & lt), ka = na + __popc(ab & lt), kr = nr + __popc(rb & lt);
    if (v) {
      if (k < kDsVCap) {
        vpos[k] = (uint16_t)pos;
        vlen[k] = (uint16_t)o.len;
      }
      const uint32_t id = cache.get(a, o);
      miss = miss || id == 0xffffffffu;
      if (o.kind == 1 && ka < x.rows) {
        x.add_actor[row0 + ka] = id;
        x.add_ctr[row0 + ka] = o.ctr;
        x.add_mem[row0 + ka] = o.mem;
      } else if (o.kind == 2 && kr < x.rows) {
        x.rm_actor[row0 + kr] = id;
        x.rm_ctr[row0 + kr] = o.ctr;
        x.rm_mem[row0 + kr] = o.mem;
      }
    }
    nv += __popc(vb);
    na += __popc(ab);
    nr += __popc(rb);
  }
  __syncthreads();
  // 4) the proven ops are the Vec's elements, back to back from the header
  bool chain = ok && nv == cnt && na <= x.rows && nr <= x.rows && gb(miss) == 0;
  for (uint32_t r = 0; __any(chain && r < nv); r += LPF) {
    const uint32_t k = r + sub;
    bool bad = false;
    if (chain && k < nv) {
      const uint32_t e = (uint32_t)vpos[k] + vlen[k];
      bad = (k == 0 && vpos[0] != p0) || (k + 1 < nv && vpos[k + 1] != e) || e > len;
    }
    chain = chain && gb(bad) == 0;
  }
  if (x.why && sub == 0 && act) {
    x.why[f] = !ok ? 1u + (nc > kDsCandCap) : nv != cnt ? 3u + (nv > cnt) * 0x100u + (nv << 16) : na > x.rows || nr > x.rows ? 4u
               : gb(miss) ? 5u : chain ? 0u : 6u;
    if (f == 0) x.why[a.n] = (cnt << 16) | (p0 << 8) | nc;
  }
  if (chain && sub == 0) {
    const size_t n = a.n;
    x.rawcnt[f] = na;
    x.rawcnt[n + f] = na;
    x.rawcnt[2 * n + f] = nr;
    x.rawcnt[3 * n + f] = nr;
    x.rawcnt[4 * n + f] = nr;
  }
  return chain;
}

#ifndef CE_V2_OPEN_UNR
#define CE_V2_OPEN_UNR 1  // the open-only / DS forms' ChaCha20 loop (C3 open 159 -> 158 us, half the code)
#endif
#ifndef CE_DS_PRIO
#define CE_DS_PRIO 2
#endif
// W = waves per SIMD the VGPR budget is sized for (LDS allows 2.5 at LPF 16, 5 at LPF 32).
// PF = the next iteration's ciphertext loads issued inside this iteration's decode (after its
// first round, with the parameters loaded one iteration earlier), so they land while the decode
// and the next iteration's first ChaCha20 block run instead of being waited for at the first
// XOR.  On for the 2-files-per-wave form only (the measured defaults, same-box A/B r02).
// ChaCha20's rot16 is two SDWA xors in every form (ce_device.h xor_rotl16_t<true>); its 9
// trailing double rounds are straight-line in the decoding forms and a rolled loop of
// CE_V2_OPEN_UNR per trip in the open-only and DS forms.
// DEC = false: open only (EncHandler::decrypt, xchacha lib.rs:73-101) -- plaintext pieces go to
// HBM at the file's out_off instead of LDS, the tag check sets the status, nothing is decoded
// (the dot-set ingest decodes the plaintext afterwards).
// DS (with DEC = false): Orswot op files of at most kDsFuseRegion bytes keep their plaintext in LDS
// and are decoded there (ds_fused_decode); larger ones, and any the decode does not prove, get
// their plaintext in HBM as in the open-only form.
template <int LPF, int W, bool PF, bool DEC = true, bool DS = false>
__global__ __launch_bounds__(64, W)
void k_open_fold_v2(DecodeArgs a) {
  static_assert(!(DEC && DS), "the DS form is an open-only form");
  static_assert(DEC || !PF, "the prefetch is issued from inside the decode");
  // ChaCha20 double rounds per loop trip (the open-only and DS forms: CE_V2_OPEN_UNR)
  constexpr int UNR = DEC ? 9 : CE_V2_OPEN_UNR;
  using C = V2Cfg<LPF>;
  constexpr int F = C::F;
  constexpr int BPL = C::BPL;
  __shared__ __attribute__((aligned(16))) uint8_t
      lds[DEC ? (F - 1) * kRegionStride2 + kRegion2 + 64 : DS ? F * kDsStride + F * kDsAuxHalves * 2 : 16];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t grp = lane / LPF, sub = lane % LPF;
  uint8_t* fl = lds + grp * (DS ? kDsStride : kRegionStride2);
  uint16_t* aux = DS ? reinterpret_cast<uint16_t*>(lds + F * kDsStride) + grp * kDsAuxHalves : nullptr;
  const uint32_t ngroups = (a.n + F - 1) / F;
  const uint32_t stride = gridDim.x;
  uint32_t g = bcast(blockIdx.x);
  // k_open_ds8's pass over the files it left: none (counters[10], counted by it) -> done
  if (DS && a.only && *reinterpret_cast<volatile const uint32_t*>(a.counters + 10) == 0) return;
  FilePre2 nx = load_pre2(a, g * F + grp);
  const SupVers sup(a);
  DecState S{38, 0, 0, 0, 0, 0xffffffffu};
  AuthFails fails;

  // 1) a file's ciphertext runs -> registers.  The 16-byte tag follows the ciphertext, so a
  //    16-byte load at any piece < npc stays inside the file; absent pieces load piece 0.
  //    Inactive lanes read the (always allocated) params array instead of the blob.
  uint4 ct[BPL][4];
  auto load_block_of = [&](const FilePre2& p, int k) {
    const bool act_ = p.ok && p.len <= kSmallMax;
    const uint32_t len_ = act_ ? p.len : 0u;
    const uint32_t npc_ = (len_ + 15) >> 4;
    const int32_t nblk_ = (int32_t)((len_ + 63) >> 6);
    const uint8_t* src_ = act_ ? a.blob + (((uint64_t)p.in_hi << 32) | p.in_off)
                               : reinterpret_cast<const uint8_t*>(a.params);
    const int32_t b = nblk_ - 1 - (int32_t)sub - LPF * k;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t q = (uint32_t)(4 * b + j);
      const uint32_t off = b >= 0 && q < npc_ ? q * 16u : 0u;
      ct[k][j] = *reinterpret_cast<const uint4*>(src_ + off);
    }
  };
  FilePre2 nn;  // PF: the parameters of the iteration after next
  if (PF) {
    // prologue: this wave's first ciphertext, and the next iteration's parameters
#pragma unroll
    for (int k = BPL - 1; k >= 0; k--) load_block_of(nx, k);
    nn = load_pre2(a, (g + stride) * F + grp);
  }

  for (; g < ngroups; g += stride) {
    const uint32_t f = g * F + grp;
    const FilePre2 cur = nx;
    if (PF) nx = nn;
    if (DS && a.only && !__any(cur.ok)) {  // a masked pass (k_open_ds8's big files): nothing here
      nx = load_pre2(a, (g + stride) * F + grp);
      continue;
    }
    const bool act = cur.ok && cur.len <= kSmallMax;
    const uint32_t len = act ? cur.len : 0u;
    const bool dsl = DS && act && len <= kDsFuseRegion;  // DS: plaintext into LDS
    const uint32_t npc = (len + 15) >> 4;             // ciphertext Poly1305 blocks
    const int32_t nblk = (int32_t)((len + 63) >> 6);  // ChaCha20 blocks
    const FileParams* Pp = a.params + (act ? f : 0);
    uint8_t* gout = DEC ? nullptr : const_cast<uint8_t*>(a.pt) + Pp->out_off;  // !DEC: plaintext in HBM

    // PF: this iteration's loads were issued during the previous one; otherwise every block's
    // loads are issued up front.
    if (!PF) {
#pragma unroll
      for (int k = BPL - 1; k >= 0; k--) load_block_of(cur, k);
    }

    // 2) per block, earliest first: keystream (counter 1 + b) in registers, XOR, plaintext ->
    //    LDS, Poly1305.  Branch-free: lanes without a block (short files) compute garbage that
    //    is neither stored where it matters nor accumulated.
    const ChachaPre cpre = chacha_pre(cur.key, 0u, cur.n2a, cur.n2b);
    L5 R1, RC;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      R1.v[i] = cur.R1[i];
      RC.v[i] = cur.R64[i];
    }
    if (LPF == 32) RC = mulmod(RC, RC);  // chain step r^(4 LPF) = r^128
    L5 R2;
#pragma unroll
    for (int i = 0; i < 5; i++) R2.v[i] = Pp->rpow[1][i];
    const MulR M1 = mul_r(R1), M2 = mul_r(R2), M3 = mul_r(mulmod(R2, R1)), MC = mul_r(RC);
    L5 acc{{0, 0, 0, 0, 0}}, glast{{0, 0, 0, 0, 0}};
    uint32_t rp[4 * C::NRP];  // r^(2^k), k <= LOG + 1
    uint4 sv4, tg4;           // s || expected tag
#pragma unroll
    for (int k = BPL - 1; k >= 0; k--) {
      const int32_t b = nblk - 1 - (int32_t)sub - LPF * k;
      const bool has = b >= 0;
      // open only: slots no file of the wave has (files under 16 x 64 B per lane slot: C3's 2 KiB
      // op files use two of the four) are skipped whole; slot 0 always has the file's last block.
      // Not in the decoding kernel: the branch splits the straight-line block sequence the
      // compiler interleaves (C2 A/B: +2-3% with it)
      if (!DEC && k > 0 && !__any(has)) continue;
      if (k == 0) {
        // the tree's powers, s and the tag: issued before the last block's ChaCha20 so their
        // latency hides under it (the other blocks' ciphertext registers are free by now)
#pragma unroll
        for (int q = 0; q < C::NRP; q++) {
          const uint4 v = *reinterpret_cast<const uint4*>(&Pp->rpow[0][0] + 4 * q);
          rp[4 * q] = v.x; rp[4 * q + 1] = v.y; rp[4 * q + 2] = v.z; rp[4 * q + 3] = v.w;
        }
        sv4 = *reinterpret_cast<const uint4*>(Pp->s);
        tg4 = *reinterpret_cast<const uint4*>(Pp->tag);
      }
      uint32_t kb[16];
      chacha_block_pre<true, UNR>(cpre, cur.key, 1u + (uint32_t)b, 0u, cur.n2a, cur.n2b, kb);
      L5 G, mj[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t q = (uint32_t)(4 * b + j);
        uint32_t xw[4] = {ct[k][j].x, ct[k][j].y, ct[k][j].z, ct[k][j].w};
        uint32_t kw[4] = {kb[4 * j], kb[4 * j + 1], kb[4 * j + 2], kb[4 * j + 3]};
        if (k == 0) {  // only lane 0's slot 0 (the file's last block) can be partial
          const uint32_t boff = q * 16u;
          const uint32_t rem = len > boff ? len - boff : 0u;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const uint32_t lo = 4 * i;
            const uint32_t keep = rem >= lo + 4 ? 0xffffffffu
                                  : (rem <= lo ? 0u : ((1u << (8 * (rem - lo))) - 1));
            xw[i] &= keep;
            kw[i] &= keep;
          }
        }
        // a lane without a block stores to bytes 4080..4095: past the end of any file that
        // has absent blocks (nblk < 64)
        const uint4 pv = make_uint4(xw[0] ^ kw[0], xw[1] ^ kw[1], xw[2] ^ kw[2], xw[3] ^ kw[3]);
        if (DEC) {
          const uint32_t st_off = has ? q * 16u : kRegion2 - 16u;
          *reinterpret_cast<uint4*>(fl + st_off) = pv;
        } else if (dsl) {
          if (has) *reinterpret_cast<uint4*>(fl + q * 16u) = pv;  // q < 4 nblk <= 128
        } else if (act && has && q * 16u < len) {
          // out_off is 16-aligned and the next file's plaintext starts >= 99 B past this one's
          // end (its header, envelope and tag), so the zero-padded tail piece is a whole store
          *reinterpret_cast<uint4*>(gout + q * 16u) = pv;
        }
        const L5 m = block_limbs(xw[0], xw[1], xw[2], xw[3]);
        if (k > 0) {
          mj[j] = m;   // a full block: Poly1305 below, one reduction for the whole block
        } else if (j == 0) {
          G = m;  // piece 4 b exists whenever the block does
        } else {
          const L5 gn = add5(mulmod(G, R1), m);
          if (k == 0) {
            const bool ex = q < npc;
#pragma unroll
            for (int i = 0; i < 5; i++) G.v[i] = ex ? gn.v[i] : G.v[i];
          } else {
            G = gn;
          }
        }
      }
      L5 an;
      if (k > 0) {
        // every block but slot 0 is full: acc r^(4 LPF) + m0 r^3 + m1 r^2 + m2 r + m3 as four
        // products into one set of column sums, carried once (vs four Horner mulmods)
        uint64_t d[5] = {mj[3].v[0], mj[3].v[1], mj[3].v[2], mj[3].v[3], mj[3].v[4]};
        mac5(d, acc, MC);
        mac5(d, mj[0], M3);
        mac5(d, mj[1], M2);
        mac5(d, mj[2], M1);
        an = reduce5(d);
      } else {
        an = add5(mulmod(acc, RC), G);
      }
      const bool to_acc = has && !(k == 0 && sub == 0);
#pragma unroll
      for (int i = 0; i < 5; i++) acc.v[i] = to_acc ? an.v[i] : acc.v[i];
      if (k == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) glast.v[i] = has && sub == 0 ? G.v[i] : 0u;
      }
    }

    // 3) chains -> tree positions (q takes lane q + 1's chain, q = LPF - 1 lane 0's), then
    //    U = sum_q v_q r^(4q) at q = 0
    const int srcl = (int)(grp * LPF + ((sub + 1) & (LPF - 1)));
    L5 v;
#pragma unroll
    for (int i = 0; i < 5; i++) v.v[i] = (uint32_t)__shfl((int)acc.v[i], srcl);
#pragma unroll
    for (int k = 0; k < C::LOG; k++) {
      L5 rk, o;
#pragma unroll
      for (int i = 0; i < 5; i++) {
        rk.v[i] = rp[5 * (k + 2) + i];
        o.v[i] = k < 4 ? row_down(v.v[i], 1 << k) : (uint32_t)__shfl_down((int)v.v[i], 16);
      }
      v = add5(v, mulmod(o, rk));  // limbs < 2^28 after 4 levels: mulmod carries in 64 bits
    }
    // T = (U r^(5 - delta) + G' r + lenblock) r; r^(5 - delta) = r^4 r, r^4, r^2 r, r^2
    const uint32_t delta = (uint32_t)(4 * nblk) - npc;
    L5 r1, base;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      r1.v[i] = rp[i];
      base.v[i] = delta < 2 ? rp[10 + i] : rp[5 + i];
    }
    const L5 br = mulmod(base, r1);
    L5 e;
#pragma unroll
    for (int i = 0; i < 5; i++) e.v[i] = (delta & 1) ? base.v[i] : br.v[i];
    const L5 y = add5(mulmod(glast, r1), block_limbs(0u, 0u, len, 0u));  // le64(0) || le64(len)
    const L5 tot = mulmod(carry5(add5(mulmod(v, e), y)), r1);
    bool tag_ok = false;
    if (act && sub == 0) {
      const uint32_t sv[4] = {sv4.x, sv4.y, sv4.z, sv4.w};
      uint32_t tag[4];
      poly_tag(tot, sv, tag);
      tag_ok = ((tag[0] ^ tg4.x) | (tag[1] ^ tg4.y) | (tag[2] ^ tg4.z) | (tag[3] ^ tg4.w)) == 0;
      if (!tag_ok) a.status[f] = CE_ERR_AUTH;
    }
    fails.add(act && sub == 0 && !tag_ok, f);
    const bool ok = grp_bits<LPF>(tag_ok, grp) != 0;

    // 4) data-version check, decode from LDS, fold; the next iteration's parameters are loaded
    //    inside (their latency hides under the decode)
    if (!DEC) {
      if (DS) {
        bool done = false;
        if (__any(dsl && ok)) {
          if (CE_DS_PRIO) __builtin_amdgcn_s_setprio(CE_DS_PRIO);  // as k_open_fold_v3's decode
          done = ds_fused_decode<LPF>(a, sup, fl, aux, len, dsl && ok, f, grp, sub);
          if (CE_DS_PRIO) __builtin_amdgcn_s_setprio(0);
        }
        if (dsl && ok && !done) {  // the lane-per-file decode reads it from HBM
          for (uint32_t q = sub; q * 16u < len; q += LPF)
            *reinterpret_cast<uint4*>(gout + q * 16u) = *reinterpret_cast<const uint4*>(fl + q * 16u);
        }
        if (sub == 0 && f < a.n && (!a.only || cur.ok)) a.ds.done[f] = done ? 1 : 0;
        __syncthreads();  // the next iteration's plaintext overwrites the regions
      }
      (void)ok;
      nx = load_pre2(a, (g + stride) * F + grp);
    } else
    decode_fold<LPF>(a, sup, fl, len, act && ok, cur.apply != 0, f, grp, sub, S, [&] {
      if (PF) {
        // next iteration's ciphertext (its parameters arrived one iteration ago) into the
        // registers this iteration no longer needs, then the parameters one further ahead
#pragma unroll
        for (int k = BPL - 1; k >= 0; k--) load_block_of(nx, k);
        nn = load_pre2(a, (g + 2 * stride) * F + grp);
      } else {
        nx = load_pre2(a, (g + stride) * F + grp);
      }
    });
    __builtin_amdgcn_wave_barrier();
  }
  fails.flush(a);
}

#ifndef CE_V3_UNR
#define CE_V3_UNR 1  // ChaCha20 double rounds per trip of chacha_block_pre's 9-trip loop: 1 keeps
#endif                // the kernel's code inside the instruction cache (9, straight-line: +2% time)
#ifndef CE_V3_PRIO
#define CE_V3_PRIO 2  // wave priority over the decode (s_setprio): the decode's short dependent
#endif                // chains issue ahead of the other wave's ChaCha20 (C2-B -10%, C2 flat)
// the Poly1305 value 1 in radix-2^26 limbs (k_open_fold_v3's weight of the lanes at q & 3 = 0 /
// q >> 2 = 0, read like the other weights)
// ---- GSet<u64> op files decoded in the open (k_open_fold_v3's GS form) ----------------------
// The third grammar beside Dot and PN: the body is a bare Vec<u64> (ce_gset.hip has the element
// grammar), decoded from the file's plaintext in LDS by its 16 lanes; members of gated files go
// to the hash tables of a.gs (gs_put: the committed table read-only, absent members claimed in
// the batch table).  Every byte used lies below the file's own length: an element is checked
// against blen before its window is read, so what an earlier group left in the region is never
// taken for this file's.
struct GsCounts {  // files by path, per lane (sub == 0 counts its group's), flushed once per wave
  uint32_t uni = 0, gen = 0;
  __device__ __forceinline__ void flush(const DecodeArgs& a) const {
    uint32_t u = uni, g = gen;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      u += (uint32_t)__shfl_xor((int)u, d);
      g += (uint32_t)__shfl_xor((int)g, d);
    }
    if ((threadIdx.x & 63) == 0) {
      if (u) atomicAdd(&a.gs->paths[0], u);
      if (g) atomicAdd(&a.gs->paths[1], g);
      if (u + g) atomicAdd(&a.gs->paths[2], u + g);
    }
  }
};

// the element at byte p of the body (p < blen): its encoded length (0: not a u64, or cut short by
// the file's end) and value.  One 12-byte window: four aligned LDS dwords, alignbyte into place.
__device__ __forceinline__ uint32_t gs_elem_lds(const uint32_t* L, uint32_t blen, uint32_t p,
                                                unsigned long long* out) {
  const LdsWin<3> W(L, p);
  const uint32_t m = W.byte(0);
  if (m <= 0x7f) {
    *out = m;
    return 1;
  }
  if (m < 0xcc || m > 0xd3) return 0;
  const uint32_t wd = 1u << ((m - 0xcc) & 3);
  if (blen - p - 1 < wd) return 0;
  const uint32_t x0 = __builtin_bswap32(W.word(1)), x1 = __builtin_bswap32(W.word(5));
  const unsigned long long x = wd == 8 ? ((unsigned long long)x0 << 32) | x1 : (unsigned long long)(x0 >> (32 - 8 * wd));
  if (m >= 0xd0 && ((x >> (8 * wd - 1)) & 1)) return 0;  // a negative integer
  *out = x;
  return 1 + wd;
}

template <int LPF, typename Pf>
__device__ __forceinline__ void decode_gset_lds(const DecodeArgs& a, const SupVers& sup, const uint8_t* fl,
                                                uint32_t len, bool live, bool apply, uint32_t f,
                                                uint32_t grp, uint32_t sub, GsCounts& C, Pf&& prefetch) {
  int32_t st = CE_OK;
  if (live) {
    if (len < 16) st = CE_ERR_PT_LEN;
    else if (!sup.has(a, *reinterpret_cast<const uint4*>(fl))) st = CE_ERR_PT_VERSION;
  }
  const uint8_t* body = fl + 16;
  const uint32_t* L = reinterpret_cast<const uint32_t*>(body);
  const uint32_t blen = len >= 16 ? len - 16 : 0;
  uint32_t cnt = 0, h = 0;
  if (live && st == CE_OK) {
    if (blen == 0) st = CE_ERR_DECODE;
    else {
      const uint32_t m = body[0];
      if ((m & 0xf0) == 0x90) { cnt = m & 15; h = 1; }
      else if (m == 0xdc && blen >= 3) { cnt = (uint32_t)body[1] << 8 | body[2]; h = 3; }
      else if (m == 0xdd && blen >= 5) {
        cnt = (uint32_t)body[1] << 24 | (uint32_t)body[2] << 16 | (uint32_t)body[3] << 8 | body[4];
        h = 5;
      } else st = CE_ERR_DECODE;
      if (st == CE_OK && cnt > blen - h) st = CE_ERR_DECODE;  // each element takes >= 1 byte
    }
  }
  prefetch();
  const bool dec = live && st == CE_OK;
  const bool ins = dec && apply;
  const GsFused* G = a.gs;
  // uniform width: the first element's marker gives w0 and count x w0 fits; lane `sub` checks the
  // marker of each element it takes (sub, sub + 16, ...).  Nothing is read as a member before
  // every lane of the group has found its markers right.
  uint32_t w0 = 0, mk = 0;
  if (dec && cnt > 0) {
    mk = body[h];
    w0 = mk <= 0x7f ? 1u : (mk >= 0xcc && mk <= 0xcf) ? 1u + (1u << (mk - 0xcc)) : 0u;
    if (w0 && (unsigned long long)cnt * w0 > blen - h) w0 = 0;
  }
  bool bad = dec && cnt > 0 && w0 == 0;
  if (w0)
    for (uint32_t e = sub; e < cnt && !bad; e += LPF) {
      const uint32_t m = body[h + e * w0];
      bad = w0 == 1 ? m > 0x7f : m != mk;
    }
  const bool general = dec && grp_bits<LPF>(bad, grp) != 0;
  if (dec && sub == 0) {
    C.uni += general ? 0u : 1u;
    C.gen += general ? 1u : 0u;
  }
  if (ins && !general) {
    // four elements of the lane at a time: their first probes of both tables are issued together
    // (eight independent loads in flight; one element at a time left the kernel waiting on each
    // probe in turn at 2 waves per SIMD).  A first probe that finds the key settles the element;
    // anything else takes gs_put's full probe.
    const GsTable ct = G->committed, bt = G->batch;
    for (uint32_t e = sub; e < cnt; e += 4 * LPF) {
      unsigned long long v[4], c[4], b[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t ej = e + (uint32_t)j * LPF;
        v[j] = 0;
        if (ej < cnt) (void)gs_elem_lds(L, blen, h + ej * w0, &v[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t hs = gs_hash(v[j]);
        c[j] = ld_slot(&ct.slots[hs & ct.mask]);
        b[j] = ld_slot(&bt.slots[hs & bt.mask]);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (e + (uint32_t)j * LPF >= cnt) continue;
        if (v[j] != 0 && (c[j] == v[j] || (c[j] == 0 && b[j] == v[j]))) continue;
        gs_put(ct, bt, v[j]);
      }
    }
  }
  // general (mixed widths, d0..d3, non-minimal forms): the group's lane 0 walks the elements
  // front to back, LPF to a round, and hands element k's offset to lane k; the lanes then read
  // and insert their own.  The rounds are wave-uniform (the groups' counts differ).
  uint32_t pos = h, remaining = general ? cnt : 0u;
  while (__any(remaining > 0 && st == CE_OK)) {
    const bool run = remaining > 0 && st == CE_OK;
    const uint32_t todo = run ? (remaining < (uint32_t)LPF ? remaining : (uint32_t)LPF) : 0u;
    uint32_t mine = 0xffffffffu;
#pragma unroll 1
    for (uint32_t k = 0; k < (uint32_t)LPF; k++) {
      uint32_t w = 0;
      unsigned long long v;
      const bool step = k < todo && st == CE_OK;
      if (step && sub == 0 && pos < blen) w = gs_elem_lds(L, blen, pos, &v);
      w = (uint32_t)__shfl((int)w, (int)(grp * LPF));
      if (step) {
        if (w == 0) st = CE_ERR_DECODE;
        else {
          if (sub == k) mine = pos;
          pos += w;
        }
      }
    }
    if (run && st == CE_OK) {
      if (ins && mine != 0xffffffffu) {
        unsigned long long v = 0;
        (void)gs_elem_lds(L, blen, mine, &v);
        gs_put(G->committed, G->batch, v);
      }
      remaining -= todo;
    }
  }
  if (live && st != CE_OK && sub == 0) {
    a.status[f] = st;
    atomicAdd(&a.counters[3], 1u);
    atomicMin(&a.counters[5], f);
  }
}

// ---- LWWReg<u64, u64> op files decoded in the open (k_open_fold_v3's LW form) ----------------
// The fourth grammar: the body is a Vec<LWWReg> (ce_lww.h has the element grammar and the fold's
// order), decoded from the file's plaintext in LDS by its 16 lanes.  Nothing is folded: the group
// leaves the file's own winner -- largest marker, lowest element index -- as one 16-byte record at
// a.lw->rec[f] (zeroed by the host: a gated-out, failing or all-marker-0 file writes nothing), and
// k_lww_reduce picks the batch's.  Rows are indexed by f, so the order in which the waves draw
// their groups cannot reach the result.  As in the GSet form every byte used lies below the
// file's own length.
struct LwCounts {  // files by path, per lane (sub == 0 counts its group's), flushed once per wave
  uint32_t uni = 0, gen = 0;
  __device__ __forceinline__ void flush(const DecodeArgs& a) const {
    uint32_t u = uni, g = gen;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      u += (uint32_t)__shfl_xor((int)u, d);
      g += (uint32_t)__shfl_xor((int)g, d);
    }
    if ((threadIdx.x & 63) == 0) {
      if (u) atomicAdd(&a.lw->paths[0], u);
      if (g) atomicAdd(&a.lw->paths[1], g);
      if (u + g) atomicAdd(&a.lw->paths[2], u + g);
    }
  }
};

__device__ __forceinline__ unsigned long long lw_shfl_xor64(unsigned long long v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
  return ((unsigned long long)hi << 32) | lo;
}

template <int LPF, typename Pf>
__device__ __forceinline__ void decode_lww_lds(const DecodeArgs& a, const SupVers& sup, const uint8_t* fl,
                                               uint32_t len, bool live, bool apply, uint32_t f,
                                               uint32_t grp, uint32_t sub, LwCounts& C, Pf&& prefetch) {
  static_assert(LPF == 16, "the group reduce below is four xor steps");
  int32_t st = CE_OK;
  if (live) {
    if (len < 16) st = CE_ERR_PT_LEN;
    else if (!sup.has(a, *reinterpret_cast<const uint4*>(fl))) st = CE_ERR_PT_VERSION;
  }
  const uint8_t* body = fl + 16;
  const uint32_t* L = reinterpret_cast<const uint32_t*>(body);
  const uint32_t blen = len >= 16 ? len - 16 : 0;
  uint32_t cnt = 0, h = 0;
  if (live && st == CE_OK) {
    if (blen == 0) st = CE_ERR_DECODE;
    else {
      const uint32_t m = body[0];
      if ((m & 0xf0) == 0x90) { cnt = m & 15; h = 1; }
      else if (m == 0xdc && blen >= 3) { cnt = (uint32_t)body[1] << 8 | body[2]; h = 3; }
      else if (m == 0xdd && blen >= 5) {
        cnt = (uint32_t)body[1] << 24 | (uint32_t)body[2] << 16 | (uint32_t)body[3] << 8 | body[4];
        h = 5;
      } else st = CE_ERR_DECODE;
      if (st == CE_OK && cnt > blen - h) st = CE_ERR_DECODE;  // each element takes >= 1 byte
    }
  }
  prefetch();
  const bool dec = live && st == CE_OK;
  // uniform stride: the first element's two integer markers give (wv, wm); count x stride fits,
  // so each of a lane's elements (sub, sub + 16, ...) lies whole inside the file -- the 5-byte
  // head, both integers and the 7-byte key -- before its windows are read.  The lane checks each
  // of them byte for byte and keeps its best (marker, index), replacing on strictly greater only:
  // its elements come in ascending order, so an equal marker keeps the earlier one.
  uint32_t wv = 0, wm = 0, stride = 0;
  if (dec && cnt > 0 && blen - h >= 14) {
    wv = lww_uint_width((uint8_t)body[h + 5]);
    if (wv && h + 12 + wv < blen) wm = lww_uint_width((uint8_t)body[h + 12 + wv]);
    if (wv && wm) stride = 12 + wv + wm;
    if (stride && (unsigned long long)cnt * stride > blen - h) stride = 0;
  }
  bool bad = dec && cnt > 0 && stride == 0;
  unsigned long long bm = 0, bv = 0;
  uint32_t bi = 0xffffffffu;
  if (stride)
    for (uint32_t e = sub; e < cnt && !bad; e += LPF) {
      const uint32_t x = h + e * stride;  // (< blen <= 4080)
      const LdsWin<4> V(L, x);            // 82 a3"val" <uint>: bytes 0 .. 5 + wv
      uint32_t lv = 0, lm = 0;
      const unsigned long long v = V.uint_at(5, &lv);
      const LdsWin<4> M(L, x + 5 + wv);   // a6"marker" <uint>: bytes 0 .. 7 + wm
      const unsigned long long m = M.uint_at(7, &lm);
      bad = V.w[0] != 0x6176a382u || V.byte(4) != 0x6cu || lv != wv || M.w[0] != 0x72616da6u ||
            (M.w[1] & 0xffffffu) != 0x72656bu || lm != wm;
      if (!bad && m > bm) { bm = m; bv = v; bi = e; }
    }
  const bool general = dec && grp_bits<LPF>(bad, grp) != 0;
  if (dec && sub == 0) {
    C.uni += general ? 0u : 1u;
    C.gen += general ? 1u : 0u;
  }
  // the group's best into each of its lanes: largest marker, then lowest element index
#pragma unroll
  for (int d = LPF / 2; d >= 1; d >>= 1) {
    const unsigned long long om = lw_shfl_xor64(bm, d), ov = lw_shfl_xor64(bv, d);
    const uint32_t oi = (uint32_t)__shfl_xor((int)bi, d);
    const bool take = om > bm || (om == bm && oi < bi);
    bm = take ? om : bm;
    bv = take ? ov : bv;
    bi = take ? oi : bi;
  }
  // general (mixed widths, the array form, another key order, unknown keys, other integer forms):
  // the group's lane 0 walks the elements front to back through the host's parser
  if (general && sub == 0) {
    bm = 0;
    bv = 0;
    Rd q{body, blen, h};
    for (uint32_t e = 0; e < cnt; e++) {
      uint64_t v = 0, m = 0;
      if (parse_lww_op(q, &v, &m) != 1) { st = CE_ERR_DECODE; break; }  // (too deep: rejected)
      if (m > bm) { bm = m; bv = v; }
    }
  }
  if (dec && st == CE_OK && apply && sub == 0 && bm != 0) a.lw->rec[f] = LwwRec{bm, bv};
  if (live && st != CE_OK && sub == 0) {
    a.status[f] = st;
    atomicAdd(&a.counters[3], 1u);
    atomicMin(&a.counters[5], f);
  }
}

__device__ const uint32_t kPolyOne[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};

// ----------------------------------------------------------------------------------------
// k_open_fold_v3: k_open_fold_v2<16, 2, false> (the C2 kernel before it) with its Poly1305 rebuilt
// around the setup's per-file constants (PolyAux, ce_kernels.h), so that every Poly1305 step
// of a lane is a four-product column sum reduced once, and the cross-lane combination is sums:
//   - the full blocks: acc r^64 + m0 r^3 + m1 r^2 + m2 r + m3 (r^3 from the setup; the first
//     block has no acc term);
//   - the file's last block (lane 0, k = 0) in the same four-product form: its Poly1305
//     pieces are loaded shifted by delta (the pieces it lacks, 4 nblk - npc), so the absent ones
//     are the leading zeros of the Horner form and the sum is G' itself; the partial piece's
//     bytes past the ciphertext (the tag's) are masked;
//   - lane s's chain sits at tree position q = s - 1 (lane 0's at 15) with weight r^(4q) =
//     r^(4 (q & 3)) r^(16 (q >> 2)): two multiplications per lane, then a DPP sum of the 16
//     lanes (v2: a four-level tree, one multiplication per level);
//   - T = U r^(6 - delta) + G' r^2 + L r (r^(6 - delta) and L r from the setup) and the check
//     against (tag - s) mod 2^128 (xchacha lib.rs:92-97).
// The plaintext past the ciphertext (the last piece's tag bytes XOR keystream) is not masked:
// the decode reads nothing past len.  ChaCha20, the LDS plaintext and the decode are v2's.
// ----------------------------------------------------------------------------------------
// PAIR: the lane's blocks' keystreams two at a time (chacha_block_pre2); EARLY: the next file's
// parameters loaded when this one starts (a whole iteration of latency) instead of in the decode
// PN: the decode's op grammar (decode_fold's PN; a.batch in two planes); the open is the same
// code.  Only k_open_fold_v3<false, true, true> is built: a PNCounter core takes no alternate.
// GS: the GSet grammar (decode_gset_lds, into the hash tables of a.gs) in place of decode_fold;
// only k_open_fold_v3<false, true, false, true> is built.  Every GS difference is an `if
// constexpr`: the other instantiations compile the code they always did.
// LW: the LWWReg grammar (decode_lww_lds, one record per file into the column of a.lw), built the
// same way; only k_open_fold_v3<false, true, false, false, true> is.
template <bool PAIR, bool EARLY, bool PN = false, bool GS = false, bool LW = false>
__global__ __launch_bounds__(64, 2)
void k_open_fold_v3(DecodeArgs a) {
  constexpr int LPF = 16, F = 4, BPL = 4;
  __shared__ __attribute__((aligned(16))) uint8_t lds[(F - 1) * kRegionStride2 + kRegion2 + 64];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t grp = lane / LPF, sub = lane % LPF;
  uint8_t* fl = lds + grp * kRegionStride2;
  // A wave takes runs of consecutive file groups (load_ops order: a writer's files are adjacent,
  // so the lane's actor cache and pending max carry over from file to file): first its fixed run
  // of `fixed` groups, CE_DYN_STATIC_PCT percent of an even share and drawn with no atomic, then
  // chunks of CE_DYN_CHUNK groups drawn from the ticket word until the batch runs out, so that a
  // wave that gets ahead takes more and every wave stays resident to the end.  Chunk t is groups
  // [dyn0 + t CE_DYN_CHUNK, + CE_DYN_CHUNK).  Lane 0 draws one chunk ahead (`tk`, its lane 0): the
  // iteration that takes a run's last group reads the ticket of the run after it (the next
  // parameters are loaded from there) and issues the atomic for the one after that, ahead of its
  // own loads.  The ticket that is read was drawn CE_DYN_CHUNK iterations before and landed long
  // ago, so reading it waits for nothing; the atomic just issued shares its latency with that
  // iteration's own parameter and ciphertext loads (vmcnt counts in order: their first wait is
  // also a wait for it), once per chunk.  What the loop carries from group to
  // group (the speculated Dot length, the actor cache, the pending (slot, max), AuthFails) are
  // caches and max-folds, right for any order of the groups.
  const uint32_t ngroups = (a.n + F - 1) / F;
  const uint32_t fixed = (uint32_t)((uint64_t)(ngroups / gridDim.x) * CE_DYN_STATIC_PCT / 100u);
  const uint32_t dyn0 = fixed * gridDim.x;
  uint32_t tk = 0;
  auto draw = [&] {
    // The word's index through an opaque VGPR: the compiler then takes the address for a per-lane
    // one and leaves the atomic as written.  With a uniform address it rewrites a uniform
    // atomicAdd into a ballot count, one lane's atomic and a broadcast, which waits for the
    // atomic's return on the spot -- the latency this draw-ahead exists to hide.
    uint32_t tw = kTicketWord;
    asm volatile("" : "+v"(tw));
    if (lane == 0) tk = atomicAdd(a.counters + tw, 1u);
  };
  auto chunk = [&](uint32_t& lo, uint32_t& hi) {  // the drawn chunk, empty at ngroups when past the end
    const uint64_t s = dyn0 + (uint64_t)bcast(tk) * CE_DYN_CHUNK;
    lo = s < ngroups ? (uint32_t)s : ngroups;
    hi = ngroups - lo < CE_DYN_CHUNK ? ngroups : lo + CE_DYN_CHUNK;
    draw();
  };
  draw();
  // gn: the group the parameters in nx belong to, the next one the loop takes; c_end: its run's end
  uint32_t gn = bcast(blockIdx.x * fixed), c_end = gn + fixed;
  if (fixed == 0) chunk(gn, c_end);
  // (tests and tools: when the wave entered the loop, stored at once so the loop carries nothing)
  if (a.stamps && lane == 0) a.stamps[(uint64_t)kStampWords * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
  FilePre2 nx = load_pre2(a, gn * F + grp);
  const SupVers sup(a);
  DecState S{PN ? 51u : 38u, 0, 0, 0, 0, 0xffffffffu};
  GsCounts gsc;
  LwCounts lwc;
  AuthFails fails;
  // this lane's tree weight r^(4q), q = (sub + 15) & 15: X = r^(4 (q & 3)) in {1, r^4, r^8,
  // r^12}, Y = r^(16 (q >> 2)) in {1, r^16, r^32, r^48}, read from FileParams.rpow / PolyAux
  // As per-lane (base, stride) address pairs, X at base + f stride (stride 0: the constant 1),
  // so the loop holds no per-lane selects or lane masks for them
  const uint32_t qpos = (sub + 15u) & 15u;
  const uint32_t qx = qpos & 3u, qy = qpos >> 2;
  static_assert(offsetof(FileParams, rpow) == 80, "rpow offset");
  auto wsrc = [&](uint32_t q, uint32_t aux_off, uint32_t rp_idx, const uint8_t*& base, uint32_t& stride) {
    base = q == 0 ? reinterpret_cast<const uint8_t*>(kPolyOne)
         : q == 3 ? reinterpret_cast<const uint8_t*>(a.aux) + aux_off
                  : reinterpret_cast<const uint8_t*>(a.params) + 80u + 20u * rp_idx;
    stride = q == 0 ? 0u : q == 3 ? (uint32_t)sizeof(PolyAux) : (uint32_t)sizeof(FileParams);
  };
  const uint8_t* x_base;
  const uint8_t* y_base;
  uint32_t x_stride, y_stride;
  wsrc(qx, (uint32_t)offsetof(PolyAux, r12), qx + 1u, x_base, x_stride);
  wsrc(qy, (uint32_t)offsetof(PolyAux, r48), qy + 3u, y_base, y_stride);

  uint4 ct[BPL][4];
  while (gn < ngroups) {
    const uint32_t f = gn * F + grp;
    const FilePre2 cur = nx;
    // the group after this one: the next of the run, or the first of the chunk drawn before
    if (++gn == c_end) chunk(gn, c_end);
    if (EARLY) nx = load_pre2(a, gn * F + grp);
    const bool act = cur.ok && cur.len <= kSmallMax;
    const uint32_t len = act ? cur.len : 0u;
    const uint32_t npc = (len + 15) >> 4;             // ciphertext Poly1305 pieces
    const int32_t nblk = (int32_t)((len + 63) >> 6);  // ChaCha20 blocks
    const FileParams* Pp = a.params + (act ? f : 0);
    const PolyAux* Xp = a.aux + (act ? f : 0);
    const uint8_t* src = act ? a.blob + (((uint64_t)cur.in_hi << 32) | cur.in_off)
                             : reinterpret_cast<const uint8_t*>(a.params);
    // 1) ciphertext -> registers, every block up front.  Block k of the lane is b = nblk - 1 -
    //    sub - 16 k; all but the file's last (lane 0, k = 0) are whole, so their four pieces are
    //    one address + immediate offsets.  A lane without the block reads the params rows (any
    //    64 readable bytes); the last block clamps its pieces to the last one (the 16-byte tag
    //    follows the ciphertext: a load at any piece < npc stays inside the file).
#pragma unroll
    for (int k = BPL - 1; k >= 0; k--) {
      const int32_t b = nblk - 1 - (int32_t)sub - LPF * k;
      if (k > 0) {
        const uint8_t* bp = b >= 0 ? src + 64u * (uint32_t)b : reinterpret_cast<const uint8_t*>(a.params);
#pragma unroll
        for (int j = 0; j < 4; j++) ct[k][j] = *reinterpret_cast<const uint4*>(bp + 16 * j);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t q = (uint32_t)(4 * b + j);
          const uint32_t off = b >= 0 ? 16u * (q < npc ? q : npc - 1u) : 0u;
          ct[0][j] = *reinterpret_cast<const uint4*>(src + off);
        }
      }
    }
    // the multipliers: r, r^2, r^3 (the four-product step), r^64 (the chain step)
    L5 R1, RC, R2, R3;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      R1.v[i] = cur.R1[i];
      RC.v[i] = cur.R64[i];
      R2.v[i] = Pp->rpow[1][i];
      R3.v[i] = Xp->r3[i];
    }
    const ChachaPre cpre = chacha_pre(cur.key, 0u, cur.n2a, cur.n2b);
    L5 acc{{0, 0, 0, 0, 0}}, glast{{0, 0, 0, 0, 0}};
    L5 X, Y, E6, LR;
    uint32_t ts[4];
    uint4 pc[4];  // lane 0: the last block's Poly1305 pieces, shifted by delta
    // lane 0's shift and its last piece's valid bytes (others: 0 and 16)
    const uint32_t dl = sub == 0 ? (uint32_t)(4 * nblk) - npc : 0u;
    const uint32_t rb = sub == 0 && npc ? len - 16u * (npc - 1u) : 16u;
    uint32_t kbn[16];  // PAIR: the keystream of block k - 1 (b + 16), computed with block k's

#pragma unroll
    for (int k = BPL - 1; k >= 0; k--) {
      const int32_t b = nblk - 1 - (int32_t)sub - LPF * k;
      const bool has = b >= 0;
      if (k == (PAIR ? 1 : 0)) {
        // issued before the last block's ChaCha20 (latency hidden under it; the other blocks'
        // ciphertext registers are free by now): the shifted pieces, the tree weights, the tail
        const int32_t b0 = nblk - 1 - (int32_t)sub;  // the lane's block k = 0
        const uint8_t* pb = b0 >= 0 ? src + 16 * (int64_t)(4 * b0 - (int32_t)dl) : src;
#pragma unroll
        for (int j = 0; j < 4; j++) pc[j] = *reinterpret_cast<const uint4*>(pb + 16 * j);
        const uint32_t fi = act ? f : 0u;
        const uint32_t* xs = reinterpret_cast<const uint32_t*>(x_base + (uint64_t)fi * x_stride);
        const uint32_t* ys = reinterpret_cast<const uint32_t*>(y_base + (uint64_t)fi * y_stride);
#pragma unroll
        for (int i = 0; i < 5; i++) {
          X.v[i] = xs[i];
          Y.v[i] = ys[i];
          E6.v[i] = Xp->e6[i];
          LR.v[i] = Xp->lr[i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) ts[i] = Xp->ts[i];
      }
      uint32_t kb[16];
      if (!PAIR) {
        chacha_block_pre<true, CE_V3_UNR>(cpre, cur.key, 1u + (uint32_t)b, 0u, cur.n2a, cur.n2b, kb);
      } else {
        if (k & 1) chacha_block_pre2<CE_V3_UNR>(cpre, cur.key, 1u + (uint32_t)b, 1u + (uint32_t)(b + LPF), 0u,
                                     cur.n2a, cur.n2b, kb, kbn);
        else {
#pragma unroll
          for (int i = 0; i < 16; i++) kb[i] = kbn[i];
        }
      }
      L5 m[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t q = (uint32_t)(4 * b + j);
        const uint4 c = ct[k][j];
        const uint4 pv = make_uint4(c.x ^ kb[4 * j], c.y ^ kb[4 * j + 1], c.z ^ kb[4 * j + 2], c.w ^ kb[4 * j + 3]);
        // a lane without a block stores to bytes 4080..4095: past the end of any file that has
        // absent blocks (nblk < 64)
        *reinterpret_cast<uint4*>(fl + (has ? q * 16u : kRegion2 - 16u)) = pv;
        if (k > 0) {
          m[j] = block_limbs(c.x, c.y, c.z, c.w);
        } else {
          // position j holds piece 4 b + j - dl (none when j < dl); the last position's bytes
          // past the ciphertext are zeroed
          uint32_t w[4] = {pc[j].x, pc[j].y, pc[j].z, pc[j].w};
          const bool pres = (uint32_t)j >= dl;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            if (j == 3) {
              const int32_t cb = (int32_t)rb - 4 * i;  // valid bytes of the word
              const uint32_t keep = cb >= 4 ? ~0u : cb <= 0 ? 0u : ((1u << (8 * cb)) - 1u);
              w[i] &= keep;
            } else {
              w[i] = pres ? w[i] : 0u;
            }
          }
          m[j] = block_limbs(w[0], w[1], w[2], w[3]);
          if (j < 3) m[j].v[4] = pres ? m[j].v[4] : 0u;
        }
      }
      // acc r^64 + m0 r^3 + m1 r^2 + m2 r + m3 as four (five) products into one set of column
      // sums, carried once.  Lane 0's last block starts from zero and is kept apart (G').
      uint64_t d[5] = {m[3].v[0], m[3].v[1], m[3].v[2], m[3].v[3], m[3].v[4]};
      if (k < BPL - 1) {  // the lane's first block has no acc term
        L5 ain = acc;
        if (k == 0) {
#pragma unroll
          for (int i = 0; i < 5; i++) ain.v[i] = sub == 0 ? 0u : acc.v[i];
        }
        mac5(d, ain, mul_r(RC));
      }
      mac5(d, m[0], mul_r(R3));
      mac5(d, m[1], mul_r(R2));
      mac5(d, m[2], mul_r(R1));
      const L5 an = reduce5(d);
      const bool to_acc = has && !(k == 0 && sub == 0);
#pragma unroll
      for (int i = 0; i < 5; i++) acc.v[i] = to_acc ? an.v[i] : acc.v[i];
      if (k == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) glast.v[i] = has && sub == 0 ? an.v[i] : 0u;
      }
    }

    // 2) U = sum_q v_q r^(4q): each chain times its weight, then the group's sum into lane 0
    L5 v = mulmod(mulmod(acc, X), Y);
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
      for (int i = 0; i < 5; i++) v.v[i] += row_down(v.v[i], 1 << k);  // limbs < 2^31
    }
    // 3) T = U r^(6 - delta) + G' r^2 + L r, checked against (tag - s) mod 2^128
    uint64_t d[5] = {LR.v[0], LR.v[1], LR.v[2], LR.v[3], LR.v[4]};
    mac5(d, v, mul_r(E6));
    mac5(d, glast, mul_r(R2));
    const L5 tot = reduce5(d);
    bool tag_ok = false;
    if (act && sub == 0) {
      tag_ok = poly_check(tot, ts);
      if (!tag_ok) a.status[f] = CE_ERR_AUTH;
    }
    fails.add(act && sub == 0 && !tag_ok, f);
    const bool ok = grp_bits<LPF>(tag_ok, grp) != 0;

    // 4) data-version check, decode from LDS, fold; the next iteration's parameters are loaded
    //    inside (their latency hides under the decode)
    if (CE_V3_PRIO) __builtin_amdgcn_s_setprio(CE_V3_PRIO);  // the decode's short dependent chains first
    if constexpr (LW) {
      decode_lww_lds<LPF>(a, sup, fl, len, act && ok, cur.apply != 0, f, grp, sub, lwc, [&] {
        if (!EARLY) nx = load_pre2(a, gn * F + grp);
      });
    } else if constexpr (GS) {
      decode_gset_lds<LPF>(a, sup, fl, len, act && ok, cur.apply != 0, f, grp, sub, gsc, [&] {
        if (!EARLY) nx = load_pre2(a, gn * F + grp);
      });
    } else {
      decode_fold<LPF, true, PN>(a, sup, fl, len, act && ok, cur.apply != 0, f, grp, sub, S, [&] {
        if (!EARLY) nx = load_pre2(a, gn * F + grp);
      });
    }
    if (CE_V3_PRIO) __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_wave_barrier();
  }
  if constexpr (LW) lwc.flush(a);
  else if constexpr (GS) gsc.flush(a);
  else flush_pending<LPF>(a, sub, S.pslot, S.pbest);
  fails.flush(a);
  if (a.stamps) {
    const unsigned long long t_out = __builtin_amdgcn_s_memrealtime();
    // HW_REG_HW_ID (wave slot, SIMD, CU, SH, SE, ...) and HW_REG_XCC_ID's low four bits
    const unsigned long long hw = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                                  ((unsigned long long)(uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);
    if (lane == 0) {
      unsigned long long* o = a.stamps + (uint64_t)kStampWords * blockIdx.x;
      o[1] = t_out;
      o[2] = hw;
    }
  }
}

// ----------------------------------------------------------------------------------------
// k_open_ds8: the DS form (Orswot op files decoded in LDS, ds_fused_decode) with 8 lanes per
// file and 8 files per wave.  C3's op files (~2 KiB, 31 ChaCha20 blocks) filled two of a 16-lane
// group's four block slots per lane, so every per-file cost of an iteration (parameters, the
// Poly1305 combination and tag, the decode's setup) was paid over half a lane's work; here a lane
// owns four blocks b = nblk - 1 - sub - 8 k of a file of at most kDsFuseRegion bytes.  Poly1305
// as k_open_fold_v3 (four-product column sums, the setup's PolyAux, weights r^(4q) =
// r^(4 (q & 3)) r^(16 (q >> 2)), q < 8, a DPP sum over the group).  A single-page file past
// kDsFuseRegion is not opened here: big[f] = 1, and the 16-lane DS kernel opens it in a second
// pass over that mask.
// ----------------------------------------------------------------------------------------
// PF: the next file's ciphertext loaded before this one's decode (into the registers the open no
// longer needs), so it lands while the decode runs instead of at the next iteration's first XOR
template <bool PF>
__global__ __launch_bounds__(64, 2)
void k_open_ds8(DecodeArgs a) {
  constexpr int LPF = 8, F = 8, BPL = 4;
  // 64 B of over-read room past a region (the decode's windows read at most 52 B past a candidate
  // below len): 8 x (2112 + 448) B = 20 KiB, two waves per SIMD as the VGPRs allow
  constexpr uint32_t kStride = kDsFuseRegion + 64;
  __shared__ __attribute__((aligned(16))) uint8_t lds[F * kStride + F * kDsAuxHalves * 2];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t grp = lane / LPF, sub = lane % LPF;
  uint8_t* fl = lds + grp * kStride;
  uint16_t* aux = reinterpret_cast<uint16_t*>(lds + F * kStride) + grp * kDsAuxHalves;
  const uint32_t ngroups = (a.n + F - 1) / F;
  const uint32_t g_end = (uint32_t)(((uint64_t)(blockIdx.x + 1) * ngroups) / gridDim.x);
  uint32_t g = bcast((uint32_t)(((uint64_t)blockIdx.x * ngroups) / gridDim.x));
  FilePre2 nx = load_pre2(a, g * F + grp);
  const SupVers sup(a);
  AuthFails fails;
  const uint32_t qpos = (sub + 7u) & 7u;
  const uint32_t qx = qpos & 3u;
  const bool x_one = qx == 0, y_one = (qpos >> 2) == 0, x_aux = qx == 3;
  const uint32_t x_off = x_aux ? (uint32_t)offsetof(PolyAux, r12) : 80u + 20u * (qx + 1u);
  uint4 ct[BPL][4];
  // a file's ciphertext -> ct: block k of the lane is b = nblk - 1 - sub - 8 k, whole but for the
  // file's last (lane 0, k = 0); a lane without the block reads the params rows
  auto load_ct = [&](const FilePre2& p) {
    const bool ac = p.ok && p.len <= kDsFuseRegion;
    const uint32_t ln = ac ? p.len : 0u;
    const uint32_t np = (ln + 15) >> 4;
    const int32_t nb = (int32_t)((ln + 63) >> 6);
    const uint8_t* sr = ac ? a.blob + (((uint64_t)p.in_hi << 32) | p.in_off) : reinterpret_cast<const uint8_t*>(a.params);
#pragma unroll
    for (int k = BPL - 1; k >= 0; k--) {
      const int32_t b = nb - 1 - (int32_t)sub - LPF * k;
      if (k > 0) {
        const uint8_t* bp = b >= 0 ? sr + 64u * (uint32_t)b : reinterpret_cast<const uint8_t*>(a.params);
#pragma unroll
        for (int j = 0; j < 4; j++) ct[k][j] = *reinterpret_cast<const uint4*>(bp + 16 * j);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t q = (uint32_t)(4 * b + j);
          const uint32_t off = b >= 0 ? 16u * (q < np ? q : np - 1u) : 0u;
          ct[0][j] = *reinterpret_cast<const uint4*>(sr + off);
        }
      }
    }
  };
  if (PF) load_ct(nx);
  for (; g < g_end; g++) {
    const uint32_t f = g * F + grp;
    const FilePre2 cur = nx;
    nx = load_pre2(a, (g + 1) * F + grp);
    const bool act0 = cur.ok && cur.len <= kSmallMax;
    const bool big = act0 && cur.len > kDsFuseRegion;
    const bool act = act0 && !big;
    const uint32_t len = act ? cur.len : 0u;
    const uint32_t npc = (len + 15) >> 4;
    const int32_t nblk = (int32_t)((len + 63) >> 6);  // <= 32
    const FileParams* Pp = a.params + (act ? f : 0);
    const PolyAux* Xp = a.aux + (act ? f : 0);
    const uint8_t* src = act ? a.blob + (((uint64_t)cur.in_hi << 32) | cur.in_off)
                             : reinterpret_cast<const uint8_t*>(a.params);
    uint8_t* gout = const_cast<uint8_t*>(a.pt) + Pp->out_off;
    if (!PF) load_ct(cur);
    L5 R1, RC, R2, R3;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      R1.v[i] = cur.R1[i];
      RC.v[i] = Pp->rpow[5][i];  // the chain step r^(4 LPF) = r^32
      R2.v[i] = Pp->rpow[1][i];
      R3.v[i] = Xp->r3[i];
    }
    const ChachaPre cpre = chacha_pre(cur.key, 0u, cur.n2a, cur.n2b);
    L5 acc{{0, 0, 0, 0, 0}}, glast{{0, 0, 0, 0, 0}};
    L5 X, Y, E6, LR;
    uint32_t ts[4];
    uint4 pc[4];
    const uint32_t dl = sub == 0 ? (uint32_t)(4 * nblk) - npc : 0u;
    const uint32_t rb = sub == 0 && npc ? len - 16u * (npc - 1u) : 16u;
#pragma unroll
    for (int k = BPL - 1; k >= 0; k--) {
      const int32_t b = nblk - 1 - (int32_t)sub - LPF * k;
      const bool has = b >= 0;
      // block slots no file of the wave has are skipped (slot 0 always has the file's last block)
      if (k > 0 && !__any(has)) continue;
      if (k == 0) {
        const uint8_t* pb = has ? src + 16 * (int64_t)(4 * b - (int32_t)dl) : src;
#pragma unroll
        for (int j = 0; j < 4; j++) pc[j] = *reinterpret_cast<const uint4*>(pb + 16 * j);
        const uint32_t* xs = reinterpret_cast<const uint32_t*>(
            (x_aux ? reinterpret_cast<const uint8_t*>(Xp) : reinterpret_cast<const uint8_t*>(Pp)) + x_off);
#pragma unroll
        for (int i = 0; i < 5; i++) {
          X.v[i] = xs[i];
          Y.v[i] = Pp->rpow[4][i];  // r^16
          E6.v[i] = Xp->e6[i];
          LR.v[i] = Xp->lr[i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) ts[i] = Xp->ts[i];
      }
      uint32_t kb[16];
      chacha_block_pre<true, CE_V2_OPEN_UNR>(cpre, cur.key, 1u + (uint32_t)b, 0u, cur.n2a, cur.n2b, kb);
      L5 m[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t q = (uint32_t)(4 * b + j);
        const uint4 c = ct[k][j];
        const uint4 pv = make_uint4(c.x ^ kb[4 * j], c.y ^ kb[4 * j + 1], c.z ^ kb[4 * j + 2], c.w ^ kb[4 * j + 3]);
        if (has) *reinterpret_cast<uint4*>(fl + q * 16u) = pv;  // q < 4 nblk <= 128
        if (k > 0) {
          m[j] = block_limbs(c.x, c.y, c.z, c.w);
        } else {
          uint32_t w[4] = {pc[j].x, pc[j].y, pc[j].z, pc[j].w};
          const bool pres = (uint32_t)j >= dl;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            if (j == 3) {
              const int32_t cb = (int32_t)rb - 4 * i;
              const uint32_t keep = cb >= 4 ? ~0u : cb <= 0 ? 0u : ((1u << (8 * cb)) - 1u);
              w[i] &= keep;
            } else {
              w[i] = pres ? w[i] : 0u;
            }
          }
          m[j] = block_limbs(w[0], w[1], w[2], w[3]);
          if (j < 3) m[j].v[4] = pres ? m[j].v[4] : 0u;
        }
      }
      uint64_t d[5] = {m[3].v[0], m[3].v[1], m[3].v[2], m[3].v[3], m[3].v[4]};
      L5 ain = acc;
      if (k == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) ain.v[i] = sub == 0 ? 0u : acc.v[i];
      }
      mac5(d, ain, mul_r(RC));  // (acc is zero before the lane's first block)
      mac5(d, m[0], mul_r(R3));
      mac5(d, m[1], mul_r(R2));
      mac5(d, m[2], mul_r(R1));
      const L5 an = reduce5(d);
      const bool to_acc = has && !(k == 0 && sub == 0);
#pragma unroll
      for (int i = 0; i < 5; i++) acc.v[i] = to_acc ? an.v[i] : acc.v[i];
      if (k == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) glast.v[i] = has && sub == 0 ? an.v[i] : 0u;
      }
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
      X.v[i] = x_one ? (i == 0 ? 1u : 0u) : X.v[i];
      Y.v[i] = y_one ? (i == 0 ? 1u : 0u) : Y.v[i];
    }
    L5 v = mulmod(mulmod(acc, X), Y);
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
      for (int i = 0; i < 5; i++) v.v[i] += row_down(v.v[i], 1 << k);
    }
    uint64_t d[5] = {LR.v[0], LR.v[1], LR.v[2], LR.v[3], LR.v[4]};
    mac5(d, v, mul_r(E6));
    mac5(d, glast, mul_r(R2));
    const L5 tot = reduce5(d);
    bool tag_ok = false;
    if (act && sub == 0) {
      tag_ok = poly_check(tot, ts);
      if (!tag_ok) a.status[f] = CE_ERR_AUTH;
    }
    fails.add(act && sub == 0 && !tag_ok, f);
    const bool ok = grp_bits<LPF>(tag_ok, grp) != 0;
    if (PF) load_ct(nx);
    bool done = false;
    if (__any(act && ok)) {
      if (CE_DS_PRIO) __builtin_amdgcn_s_setprio(CE_DS_PRIO);
      done = ds_fused_decode<LPF>(a, sup, fl, aux, len, act && ok, f, grp, sub);
      if (CE_DS_PRIO) __builtin_amdgcn_s_setprio(0);
    }
    if (act && ok && !done) {  // the lane-per-file decode reads it from HBM
      for (uint32_t q = sub; q * 16u < len; q += LPF)
        *reinterpret_cast<uint4*>(gout + q * 16u) = *reinterpret_cast<const uint4*>(fl + q * 16u);
    }
    if (sub == 0 && f < a.n) {
      a.ds.done[f] = done ? 1 : 0;
      a.ds.big[f] = big ? 1 : 0;
    }
    // big files counted (counters[10], zeroed with the block before the open): the 16-lane pass
    // over them returns at once when there are none
    const unsigned long long bb = __ballot(big && sub == 0);
    if (bb && lane == (uint32_t)__builtin_ctzll(bb)) atomicAdd(&a.counters[10], (uint32_t)__builtin_popcountll(bb));
    __syncthreads();  // the next iteration's plaintext overwrites the regions
  }
  fails.flush(a);
}

template <int LPF, int W, bool PF, bool DEC = true, bool DS = false>
static void launch_v2(hipStream_t s, const DecodeArgs& a, OpenLaunchLog& log, const char* key,
                      hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
  static const uint32_t res = resident_blocks(k_open_fold_v2<LPF, W, PF, DEC, DS>, 64);
  const uint32_t groups = (a.n + 64 / LPF - 1) / (64 / LPF);
  const dim3 grid(log.grid(std::min<uint32_t>(groups, res), key));
  if (t0) {  // the launch's own start / end timestamps: no marker packets around the kernel
    hipExtLaunchKernelGGL((k_open_fold_v2<LPF, W, PF, DEC, DS>), grid, dim3(64), 0, s, t0, t1, 0u, a);
  } else {
    hipLaunchKernelGGL((k_open_fold_v2<LPF, W, PF, DEC, DS>), grid, dim3(64), 0, s, a);
  }
}

// single-page files opened into HBM (a.pt at each file's out_off), lane-owned ChaCha20 blocks;
// a.only / a.apply unused.  Larger files: k_segments with skip_small (their setup's list).
hipError_t launch_open_small_v2(hipStream_t s, const DecodeArgs& a, OpenLaunchLog& log) {
  if (a.n == 0) return hipSuccess;
  // The DS form: 8 lanes per file for files of at most kDsFuseRegion bytes (k_open_ds8, with the
  // setup's PolyAux), then the 16-lane DS form over the files it left (a.only = big; it returns
  // at once when there are none).  CE_DS8=0: the 16-lane form for every file (A/B).  Measured at
  // C3 (r06, same box, rocprofv3): 65.0K VALU lane-instr per file against 79.7K; with both
  // kernels' ChaCha20 rolled and the decode at raised wave priority, 143.5 us against 150.8 us
  // (before: 153-155 against 159-162, the decode's LDS and table latencies exposed at 2 waves per
  // SIMD).  The 16-lane DS form at a 3-wave VGPR budget (168, a few spills): same-box A/B against
  // 2 waves (191 VGPRs, none): 155 vs 162 us at C3 (r05)
  static const bool ds8_on = !(getenv("CE_DS8") && atoi(getenv("CE_DS8")) == 0);
  if (a.ds.on && a.aux && a.ds.big && ds8_on) {
    static const bool pf = !(getenv("CE_DS8_PF") && atoi(getenv("CE_DS8_PF")) == 0);
    if (pf) {
      static const uint32_t res = resident_blocks(k_open_ds8<true>, 64);
      const dim3 grid(log.grid(std::min<uint32_t>((a.n + 7) / 8, res), "open_ds8_pf"));
      hipLaunchKernelGGL(k_open_ds8<true>, grid, dim3(64), 0, s, a);
    } else {
      static const uint32_t res = resident_blocks(k_open_ds8<false>, 64);
      const dim3 grid(log.grid(std::min<uint32_t>((a.n + 7) / 8, res), "open_ds8_nopf"));
      hipLaunchKernelGGL(k_open_ds8<false>, grid, dim3(64), 0, s, a);
    }
    DecodeArgs b = a;
    b.only = a.ds.big;
    launch_v2<16, 3, false, false, true>(s, b, log, "open_ds16");
  } else if (a.ds.on) {
    launch_v2<16, 3, false, false, true>(s, a, log, "open_ds16");
  } else {
    launch_v2<16, 3, false, false>(s, a, log, "open_only_lpf16");
  }
  return hipGetLastError();
}

hipError_t launch_open_fold_pn(hipStream_t s, const DecodeArgs& a, OpenLaunchLog& log, hipEvent_t t0,
                               hipEvent_t t1) {
  if (a.n == 0) return hipSuccess;
  if (!a.aux) return hipErrorInvalidValue;  // the v3 open needs the setup's PolyAux rows
  static const uint32_t res = resident_blocks(k_open_fold_v3<false, true, true>, 64);
  const dim3 grid(log.grid(std::min<uint32_t>((a.n + 3) / 4, res), "open_v3_pn"));
  const DecodeArgs b = log.stamped(a, grid.x);
  if (t0) hipExtLaunchKernelGGL((k_open_fold_v3<false, true, true>), grid, dim3(64), 0, s, t0, t1, 0u, b);
  else hipLaunchKernelGGL((k_open_fold_v3<false, true, true>), grid, dim3(64), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_open_fold_gset(hipStream_t s, const DecodeArgs& a, OpenLaunchLog& log, hipEvent_t t0,
                                 hipEvent_t t1) {
  if (a.n == 0) return hipSuccess;
  if (!a.aux || !a.gs) return hipErrorInvalidValue;  // the setup's PolyAux rows, the hash tables
  static const uint32_t res = resident_blocks(k_open_fold_v3<false, true, false, true>, 64);
  const dim3 grid(log.grid(std::min<uint32_t>((a.n + 3) / 4, res), "open_v3_gset"));
  const DecodeArgs b = log.stamped(a, grid.x);
  if (t0) hipExtLaunchKernelGGL((k_open_fold_v3<false, true, false, true>), grid, dim3(64), 0, s, t0, t1, 0u, b);
  else hipLaunchKernelGGL((k_open_fold_v3<false, true, false, true>), grid, dim3(64), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_open_fold_lww(hipStream_t s, const DecodeArgs& a, OpenLaunchLog& log, hipEvent_t t0,
                                hipEvent_t t1) {
  if (a.n == 0) return hipSuccess;
  if (!a.aux || !a.lw) return hipErrorInvalidValue;  // the setup's PolyAux rows, the record column
  static const uint32_t res = resident_blocks(k_open_fold_v3<false, true, false, false, true>, 64);
  const dim3 grid(log.grid(std::min<uint32_t>((a.n + 3) / 4, res), "open_v3_lww"));
  const DecodeArgs b = log.stamped(a, grid.x);
  if (t0) hipExtLaunchKernelGGL((k_open_fold_v3<false, true, false, false, true>), grid, dim3(64), 0, s, t0, t1, 0u, b);
  else hipLaunchKernelGGL((k_open_fold_v3<false, true, false, false, true>), grid, dim3(64), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_open_fold_v2(hipStream_t s, const DecodeArgs& a, int files_per_wave, OpenLaunchLog& log,
                               hipEvent_t t0, hipEvent_t t1) {
  if (a.n == 0) return hipSuccess;
  // the v3 Poly1305 form (needs the setup's PolyAux rows); CE_FUSED_V2=1 keeps v2 for A/B
  static const bool force_v2 = getenv("CE_FUSED_V2") != nullptr;
  if (files_per_wave == 4 && a.aux && !force_v2) {
    // CE_V3=<bits> (A/B of correct variants): 1 = PAIR, 2 = EARLY; default 2 (same box, two runs
    // each: EARLY 2.899 / 2.859 ms against 2.913 / 2.893, PAIR 2.961 / 2.922)
    static const int v3 = [] {
      const char* e = getenv("CE_V3");
      return e ? atoi(e) : 2;
    }();
    auto go = [&](auto kern, const char* key) {
      const uint32_t res = resident_blocks(kern, 64);
      const dim3 grid(log.grid(std::min<uint32_t>((a.n + 3) / 4, res), key));
      const DecodeArgs b = log.stamped(a, grid.x);
      if (t0) hipExtLaunchKernelGGL(kern, grid, dim3(64), 0, s, t0, t1, 0u, b);
      else hipLaunchKernelGGL(kern, grid, dim3(64), 0, s, b);
    };
    switch (v3 & 3) {
      case 1: go(k_open_fold_v3<true, false>, "open_v3_p1e0"); break;
      case 2: go(k_open_fold_v3<false, true>, "open_v3_p0e1"); break;
      case 3: go(k_open_fold_v3<true, true>, "open_v3_p1e1"); break;
      default: go(k_open_fold_v3<false, false>, "open_v3_p0e0"); break;
    }
    return hipGetLastError();
  }
  // the measured defaults: next-ciphertext prefetch off at 4 files per wave (same-box A/B r02);
  // 2 files per wave at a 3-wave budget with the prefetch for the fpw = 2 geometry
  if (files_per_wave == 2) launch_v2<32, 3, true>(s, a, log, "open_v2_lpf32", t0, t1);
  else launch_v2<16, 2, false>(s, a, log, "open_v2_lpf16", t0, t1);
  return hipGetLastError();
}

// ----------------------------------------------------------------------------------------
// device version gate (crdt-enc/src/lib.rs:519-538) for batches in load_ops order
// ----------------------------------------------------------------------------------------
__global__ void k_gate_runs(GateArgs g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n) return;
  const uint32_t a = g.fa[i];
  if (a >= g.m) { atomicOr(&g.flags[0], 1u); return; }
  if (i == 0 || g.fa[i - 1] != a) {
    if (atomicAdd(&g.run_count[a], 1u) != 0) atomicOr(&g.flags[0], 1u);  // actor split
    g.run_first[a] = i;
    // consecutive run starting at version vf: a gap iff vf > expected (at the run's first
    // file).  An actor split across runs flags [0] above, and the host gate then decides alone.
    if (g.fv[i] > g.e0[a]) atomicMin(&g.flags[1], i);
  } else if (g.fv[i] != g.fv[i - 1] + 1) {
    atomicOr(&g.flags[0], 1u);  // versions not consecutive: host gate
  }
}

__global__ void k_gate_apply(GateArgs g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n) return;
  const uint32_t a = g.fa[i];
  bool ap = false;
  if (a < g.m) {
    const uint64_t e0 = g.e0[a];
    const uint64_t vf = g.fv[g.run_first[a]];
    const uint32_t gap = g.flags[1];
    ap = g.fv[i] >= e0 && vf <= e0 && i < gap;
    // versions are consecutive inside a run: only the run's last applied file bumps
    // next_op_versions (one atomic per actor instead of one per file)
    const bool last = i + 1 == g.n || g.fa[i + 1] != a || i + 1 >= gap;
    if (ap && last) {
      atomicMax(&g.newnov[a], (unsigned long long)(g.fv[i] + 1));
      if (g.newnov_host) g.newnov_host[a] = g.fv[i] + 1;
    }
  }
  g.apply[i] = ap ? 1 : 0;
}

hipError_t launch_gate(hipStream_t s, const GateArgs& g) {
  if (g.n == 0) return hipSuccess;
  const uint32_t blocks = (g.n + 255) / 256;
  hipLaunchKernelGGL(k_gate_runs, dim3(blocks), dim3(256), 0, s, g);
  hipLaunchKernelGGL(k_gate_apply, dim3(blocks), dim3(256), 0, s, g);
  return hipGetLastError();
}

}  // namespace ce
