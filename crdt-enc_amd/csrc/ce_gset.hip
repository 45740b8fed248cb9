// ce_gset.hip -- GSet<u64> on the device (gfx950): the u64 hash set (ce_gset.h) and the
// wave-per-file decode of an op file's Vec<u64> from plaintext in HBM.
//
// Element grammar (oracle/crdts.py _u64 over rmp's integer forms): positive fixint, cc / cd / ce /
// cf, and d0..d3 with a non-negative value; every other marker, and an element cut short by the
// end of the file, is CE_ERR_DECODE.  Bytes after the array are ignored.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_gset.h"
#include "ce_gset_device.h"

namespace ce {
namespace {

constexpr int kWaves = 4;  // waves per block

// the element at body[p]: its encoded length (0: invalid or cut short) and value
__device__ uint32_t gs_elem(const uint8_t* body, uint32_t blen, uint32_t p, unsigned long long* out) {
  if (p >= blen) return 0;
  const uint32_t m = body[p];
  if (m <= 0x7f) {
    *out = m;
    return 1;
  }
  if (m < 0xcc || m > 0xd3) return 0;
  const bool sgn = m >= 0xd0;
  const uint32_t w = 1u << ((m - 0xcc) & 3);
  if (blen - p - 1 < w) return 0;
  unsigned long long x = 0;
  for (uint32_t k = 0; k < w; k++) x = (x << 8) | body[p + 1 + k];
  if (sgn && ((x >> (8 * w - 1)) & 1)) return 0;  // a negative integer
  *out = x;
  return 1 + w;
}

__device__ void decode_gset_file(const GsDecodeArgs& a, uint32_t f, uint32_t lane) {
  const FileParams* Pp = a.params + f;
  const uint8_t* pt = a.pt + Pp->out_off;
  const uint32_t len = Pp->len;
  int32_t st = CE_OK;
  // clear text = VersionBytes(data_version, msgpack(Vec<u64>)) (crdt-enc/src/lib.rs:504-507)
  if (len < 16) st = CE_ERR_PT_LEN;
  else {
    const uint4 dv = *reinterpret_cast<const uint4*>(pt);
    bool found = false;
    for (uint32_t s = 0; s < a.n_supported; s++) {
      const uint4 sv = *reinterpret_cast<const uint4*>(a.supported + 16 * s);
      found |= dv.x == sv.x && dv.y == sv.y && dv.z == sv.z && dv.w == sv.w;
    }
    if (!found) st = CE_ERR_PT_VERSION;
  }
  const bool ins = st == CE_OK && a.apply[f];
  auto put = [&](unsigned long long v) { gs_put(a.committed, a.batch, v); };
  if (st == CE_OK) {
    const uint8_t* body = pt + 16;
    const uint32_t blen = len - 16;
    uint32_t cnt = 0, h = 0;
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
    if (st == CE_OK) {
      // uniform width: every element has the first one's marker (any positive fixint for a
      // fixint), and count x width fits.  Lane L checks the markers of elements L, L + 64, ...
      uint32_t w0 = 0, mk = 0;
      if (cnt > 0) {
        mk = body[h];
        w0 = mk <= 0x7f ? 1u : (mk >= 0xcc && mk <= 0xcf) ? 1u + (1u << (mk - 0xcc)) : 0u;
        if (w0 && (unsigned long long)cnt * w0 > blen - h) w0 = 0;
      }
      bool ok = w0 != 0;
      if (w0)
        for (uint32_t e = lane; e < cnt && ok; e += 64) {
          const uint32_t m = body[h + e * w0];
          ok = w0 == 1 ? m <= 0x7f : m == mk;
        }
      const bool uniform = cnt == 0 || __ballot(ok) == ~0ull;
      if (uniform) {
        if (lane == 0) atomicAdd(&a.paths[0], 1u);
        if (ins) {
          for (uint32_t e = lane; e < cnt; e += 64) {
            unsigned long long v = 0;
            (void)gs_elem(body, blen, h + e * w0, &v);
            put(v);
          }
        }
      } else {
        // general: lane 0 walks the elements front to back, 64 to a round, and hands element k's
        // position to lane k; the lanes then read and insert their own.  Members of a file that
        // fails further on land in the batch table only, which a rejected batch clears.
        if (lane == 0) atomicAdd(&a.paths[1], 1u);
        uint32_t pos = h, remaining = cnt;
        while (remaining > 0 && st == CE_OK) {
          const uint32_t todo = remaining < 64 ? remaining : 64;
          uint32_t mine = 0xffffffffu;
          for (uint32_t k = 0; k < todo; k++) {
            uint32_t w = 0;
            unsigned long long v;
            if (lane == 0) w = gs_elem(body, blen, pos, &v);
            w = (uint32_t)__shfl((int)w, 0);
            if (w == 0) { st = CE_ERR_DECODE; break; }
            if (lane == k) mine = pos;
            pos += w;
          }
          if (st != CE_OK) break;
          if (ins && mine != 0xffffffffu) {
            unsigned long long v = 0;
            (void)gs_elem(body, blen, mine, &v);
            put(v);
          }
          remaining -= todo;
        }
      }
    }
  }
  if (st != CE_OK && lane == 0) a.status[f] = st;
}

__global__ __launch_bounds__(256) void k_decode_gset(GsDecodeArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t stride = gridDim.x * kWaves;
  for (uint32_t f = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6)); f < a.n; f += stride) {
    if (a.only && !a.only[f]) continue;
    if (a.large_only && a.params[f].len <= kSmallMax) continue;  // (the fused open decoded those)
    if (a.status[f] != CE_OK) continue;
    decode_gset_file(a, f, lane);
  }
}

__global__ __launch_bounds__(256) void k_gs_insert(GsTable t, const unsigned long long* keys, uint32_t n) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) gs_insert(t, keys[i]);
}

// up to kGsMaxParts columns into t in one launch: a grid-stride loop over their concatenation,
// the part boundaries (a prefix array) and base pointers staged once into LDS, a lane's part found
// by a binary search over the prefix.  Four elements per lane and round: their keys, then their
// first probes, are issued together (the fused open's uniform path does the same); a first probe
// that finds the key settles the element, anything else takes gs_insert's full probe and claim.
__global__ __launch_bounds__(256) void k_gs_insert_parts(GsTable t, GsParts ps) {
  __shared__ uint32_t s_pre[kGsMaxParts + 1];
  __shared__ const unsigned long long* s_ptr[kGsMaxParts];
  if (threadIdx.x <= ps.k) s_pre[threadIdx.x] = ps.pre[threadIdx.x];
  if (threadIdx.x < ps.k) s_ptr[threadIdx.x] = ps.part[threadIdx.x];
  __syncthreads();
  const uint32_t total = ps.pre[ps.k];
  const uint32_t stride = gridDim.x * 256;
  // (base <= total - 1 and 4 * stride <= 2^22, the sum below stays far from 2^32: total <= 2^31)
  for (uint32_t base = blockIdx.x * 256 + threadIdx.x; base < total; base += 4 * stride) {
    unsigned long long v[4], s[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t i = base + (uint32_t)j * stride;
      v[j] = 0;
      if (i < total) {
        // the last part with pre[p] <= i (empty parts share a boundary and are skipped by it)
        uint32_t lo = 0, hi = ps.k;
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_pre[mid] <= i) lo = mid;
          else hi = mid;
        }
        v[j] = s_ptr[lo][i - s_pre[lo]];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) s[j] = ld_slot(&t.slots[gs_hash(v[j]) & t.mask]);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (base + (uint32_t)j * stride >= total) continue;
      if (v[j] != 0 && s[j] == v[j]) continue;
      gs_insert(t, v[j]);
    }
  }
}

// ---- the state-file reader: a StateWrapper's `value` array decoded from plaintext in HBM --------
// The body is taken when its elements are unsigned markers whose widths never decrease: runs of
// positive fixints (1 byte), cc (2), cd (3), ce (5) and cf (9), any of them empty.  Phase p proves
// run p: with the run starting at (element s, byte o) -- both read from the earlier phases' lengths
// -- it ends at the first t for which the byte at o + w t is not the run's marker class, the
// element would pass the end of the file, or s + t is the array's count.  Every t before it has
// then been checked marker by marker, so the first mismatch is all that counts: an atomicMin.
__device__ __forceinline__ uint32_t gs_run_width(uint32_t r) { return r == 0 ? 1u : r == 1 ? 2u : r == 2 ? 3u : r == 3 ? 5u : 9u; }

__global__ __launch_bounds__(256) void k_gs_state_runs(const uint8_t* base, const GsStateFile* files, uint32_t n,
                                                       uint32_t* runs, uint32_t phase) {
  const uint32_t w = gs_run_width(phase);
  const uint32_t stride = gridDim.x * 256;
  for (uint32_t f = blockIdx.y; f < n; f += gridDim.y) {
    const GsStateFile F = files[f];
    uint32_t* R = runs + kGsStateRunWords * f;
    uint32_t s = 0;
    unsigned long long o = 0;
    for (uint32_t k = 0; k < phase; k++) {  // (the earlier launches' results)
      const uint32_t L = R[k];
      s += L;
      o += (unsigned long long)L * gs_run_width(k);
    }
    const uint32_t rem = F.count - s;  // (a run never passes the count: s <= count)
    const uint8_t* body = base + F.body;
    // t = rem is the mismatch that always exists; count < 2^29, so t + stride cannot wrap
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t <= rem; t += stride) {
      if (t >= ld_word(&R[phase])) break;  // an earlier mismatch is known: nothing from here on counts
      bool bad = t == rem;
      if (!bad) {
        const unsigned long long pos = o + (unsigned long long)w * t;
        if (pos + w > F.blen) bad = true;  // (checked before the load: no byte past the file is read)
        else {
          const uint32_t m = body[pos];
          bad = phase == 0 ? m > 0x7f : m != 0xcbu + phase;
        }
      }
      if (bad) {
        // (looked at again after the marker's load: in a phase whose run is empty nearly every
        // candidate mismatches, and all but the first few find a smaller t already there)
        if (t < ld_word(&R[phase])) atomicMin(&R[phase], t);
        break;  // (this thread's later t are larger)
      }
    }
  }
}

// the members of up to kGsStateMaxFiles proven files into t in one launch, as k_gs_insert_parts
// takes its columns: a grid-stride loop over the files' concatenation, the element prefix and each
// file's run table (first element and first byte of every run) staged in LDS, a lane's file by a
// binary search, its run by the five starts, the element's offset in closed form.  Four elements
// per lane and round, their payloads, then their first probes, issued together.
__global__ __launch_bounds__(256) void k_gs_state_insert(GsTable t, const uint8_t* base, const GsStateFile* files,
                                                         uint32_t k, const uint32_t* runs) {
  __shared__ uint32_t s_pre[kGsStateMaxFiles + 1];
  __shared__ unsigned long long s_body[kGsStateMaxFiles];
  __shared__ uint32_t s_rs[kGsStateMaxFiles][5], s_ro[kGsStateMaxFiles][5];
  if (threadIdx.x < k) {
    const GsStateFile F = files[threadIdx.x];
    s_pre[threadIdx.x] = F.pre;
    if (threadIdx.x == k - 1) s_pre[k] = F.pre + F.count;
    s_body[threadIdx.x] = F.body;
    uint32_t s = 0, o = 0;  // (a proven file's run ends lie inside it: o <= blen < 2^32)
    for (uint32_t r = 0; r < 5; r++) {
      s_rs[threadIdx.x][r] = s;
      s_ro[threadIdx.x][r] = o;
      const uint32_t L = runs[kGsStateRunWords * threadIdx.x + r];
      s += L;
      o += L * gs_run_width(r);
    }
  }
  __syncthreads();
  const uint32_t total = s_pre[k];
  const uint32_t stride = gridDim.x * 256;
  for (uint32_t i0 = blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += 4 * stride) {
    unsigned long long v[4], s[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t i = i0 + (uint32_t)j * stride;
      v[j] = 0;
      if (i < total) {
        // the last file with pre <= i (files without members share a boundary and are skipped by it)
        uint32_t lo = 0, hi = k;
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_pre[mid] <= i) lo = mid;
          else hi = mid;
        }
        const uint32_t e = i - s_pre[lo];
        uint32_t r = 0;  // the last run that starts at or before e (empty runs share a start)
#pragma unroll
        for (uint32_t q = 1; q < 5; q++)
          if (s_rs[lo][q] <= e) r = q;
        const uint32_t w = gs_run_width(r);
        const uint8_t* p = base + s_body[lo] + s_ro[lo][r] + (unsigned long long)(e - s_rs[lo][r]) * w;
        unsigned long long x = 0;
        if (w == 1) x = p[0];
        else
          for (uint32_t b = 1; b < w; b++) x = (x << 8) | p[b];
        v[j] = x;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) s[j] = ld_slot(&t.slots[gs_hash(v[j]) & t.mask]);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (i0 + (uint32_t)j * stride >= total) continue;
      if (v[j] != 0 && s[j] == v[j]) continue;
      gs_insert(t, v[j]);
    }
  }
}

__global__ __launch_bounds__(256) void k_gs_move(GsTable src, GsTable dst) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && src.meta[kGsZero]) gs_insert(dst, 0);
  const uint32_t cap = src.mask + 1;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < cap; i += gridDim.x * 256) {
    const unsigned long long v = src.slots[i];
    if (v) gs_insert(dst, v);
  }
}

__global__ __launch_bounds__(256) void k_gs_collect(GsTable t, unsigned long long* out, uint32_t* n_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && t.meta[kGsZero]) out[atomicAdd(n_out, 1u)] = 0;
  const uint32_t cap = t.mask + 1;
  // one atomicAdd per wave and round: the wave's live slots take consecutive places
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < cap; i += gridDim.x * 256) {
    const unsigned long long v = t.slots[i];
    const unsigned long long m = __ballot(v != 0);
    if (m == 0) continue;
    const int leader = __builtin_ctzll(m);
    uint32_t base = 0;
    if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(n_out, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    if (v) out[base + (uint32_t)__popcll(m & ((1ull << (threadIdx.x & 63)) - 1))] = v;
  }
}

// GSet::contains for a column of queries against the committed table: out[i] = 1 or 0.  A probe is
// one random 8-byte read of a table far larger than L2, and a lane that waits for one before it
// issues the next pays the whole miss each time: a lane takes kGsProbes queries per round, their
// keys, then their first slots, issued together before any is looked at.  Only the first slot can
// be issued ahead; a collision walks on in gs_contains.  The member 0 is held out of band.
constexpr int kGsProbes = 8;

__global__ __launch_bounds__(256) void k_gs_contains(GsTable t, const unsigned long long* q, unsigned long long n,
                                                     uint8_t* out) {
  const uint8_t zero = ld_word(&t.meta[kGsZero]) ? 1 : 0;
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  for (unsigned long long base = (unsigned long long)blockIdx.x * 256 + threadIdx.x; base < n;
       base += kGsProbes * stride) {
    unsigned long long v[kGsProbes], s[kGsProbes];
#pragma unroll
    for (int j = 0; j < kGsProbes; j++) {
      const unsigned long long i = base + (unsigned long long)j * stride;
      v[j] = i < n ? q[i] : 0ull;
    }
    // (a lane past the end probes the slot of key 0: inside the table, never looked at)
#pragma unroll
    for (int j = 0; j < kGsProbes; j++) s[j] = ld_slot(&t.slots[gs_hash(v[j]) & t.mask]);
#pragma unroll
    for (int j = 0; j < kGsProbes; j++) {
      const unsigned long long i = base + (unsigned long long)j * stride;
      if (i >= n) continue;
      uint8_t r;
      if (v[j] == 0) r = zero;
      else if (s[j] == v[j]) r = 1;
      else if (s[j] == 0) r = 0;
      else r = gs_contains(t, v[j]) ? 1 : 0;  // (a collision: the rest of the run)
      out[i] = r;
    }
  }
}

// the serializer: an element's encoded length (uint_width: its smallest unsigned form), and the writer
__global__ __launch_bounds__(256) void k_gs_widths(const unsigned long long* v, uint32_t n, uint32_t* w) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) w[i] = uint_width(v[i]);
}

// element i at out[off[i]]; the last element's thread writes the clear length (head_len + the
// elements' bytes) where the seal reads it
__global__ __launch_bounds__(256) void k_gs_write(const unsigned long long* v, const uint32_t* off, uint32_t n,
                                                  uint8_t* out, unsigned long long* clear_len_at,
                                                  unsigned long long head_len) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned long long x = v[i];
    const uint32_t w = uint_width(x);
    uint8_t* p = out + off[i];
    if (w == 1) p[0] = (uint8_t)x;
    else {
      p[0] = (uint8_t)(w == 2 ? 0xcc : w == 3 ? 0xcd : w == 5 ? 0xce : 0xcf);
      for (uint32_t k = 1; k < w; k++) p[k] = (uint8_t)(x >> (8 * (w - 1 - k)));
    }
    if (i == n - 1) *clear_len_at = head_len + off[i] + w;
  }
}

uint32_t blocks_for(uint32_t n) {
  const uint32_t b = (n + 255) / 256;
  return b < 1 ? 1 : (b > 4096 ? 4096 : b);
}

}  // namespace

hipError_t launch_decode_gset(hipStream_t s, const GsDecodeArgs& a, uint32_t grid_waves) {
  if (a.n == 0) return hipSuccess;
  const uint32_t blocks = (grid_waves + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(k_decode_gset, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gs_insert(hipStream_t s, GsTable t, const unsigned long long* keys, uint32_t n) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gs_insert, dim3(blocks_for(n)), dim3(256), 0, s, t, keys, n);
  return hipGetLastError();
}

hipError_t launch_gs_insert_parts(hipStream_t s, GsTable t, const GsParts& ps) {
  if (ps.k == 0 || ps.pre[ps.k] == 0) return hipSuccess;
  // four elements per lane and round
  hipLaunchKernelGGL(k_gs_insert_parts, dim3(blocks_for((ps.pre[ps.k] + 3) / 4)), dim3(256), 0, s, t, ps);
  return hipGetLastError();
}

hipError_t launch_gs_state_runs(hipStream_t s, const uint8_t* base, const GsStateFile* files, uint32_t n,
                                uint32_t max_count, uint32_t* runs) {
  if (n == 0) return hipSuccess;
  // (t runs to the count inclusive; the grid's x covers the longest file, y the files)
  const uint32_t gy = n < 64 ? n : 64;
  uint32_t gx = blocks_for(max_count + 1);
  if (gx > 4096 / gy) gx = 4096 / gy;
  for (uint32_t phase = 0; phase < 5; phase++) {
    hipLaunchKernelGGL(k_gs_state_runs, dim3(gx, gy), dim3(256), 0, s, base, files, n, runs, phase);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

hipError_t launch_gs_state_insert(hipStream_t s, GsTable t, const uint8_t* base, const GsStateFile* files, uint32_t k,
                                  uint32_t total, const uint32_t* runs) {
  if (k == 0 || total == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gs_state_insert, dim3(blocks_for((total + 3) / 4)), dim3(256), 0, s, t, base, files, k, runs);
  return hipGetLastError();
}

hipError_t launch_gs_move(hipStream_t s, GsTable src, GsTable dst) {
  hipLaunchKernelGGL(k_gs_move, dim3(blocks_for(src.mask + 1)), dim3(256), 0, s, src, dst);
  return hipGetLastError();
}

hipError_t launch_gs_widths(hipStream_t s, const unsigned long long* v, uint32_t n, uint32_t* w) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gs_widths, dim3(blocks_for(n)), dim3(256), 0, s, v, n, w);
  return hipGetLastError();
}

hipError_t launch_gs_write(hipStream_t s, const unsigned long long* v, const uint32_t* off, uint32_t n, uint8_t* out,
                           unsigned long long* clear_len_at, uint64_t head_len) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gs_write, dim3(blocks_for(n)), dim3(256), 0, s, v, off, n, out, clear_len_at,
                     (unsigned long long)head_len);
  return hipGetLastError();
}

hipError_t launch_gs_contains(hipStream_t s, GsTable t, const unsigned long long* q, uint64_t n, uint8_t* out,
                              uint32_t grid_cap) {
  if (n == 0) return hipSuccess;
  const uint64_t per = 256 * kGsProbes;  // queries a block takes per trip of its loop
  uint64_t blocks = (n + per - 1) / per;
  const uint32_t cap = grid_cap ? grid_cap : 2048;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k_gs_contains, dim3((uint32_t)blocks), dim3(256), 0, s, t, q, (unsigned long long)n, out);
  return hipGetLastError();
}

hipError_t launch_gs_collect(hipStream_t s, GsTable t, unsigned long long* out, uint32_t* n_out) {
  hipLaunchKernelGGL(k_gs_collect, dim3(blocks_for(t.mask + 1)), dim3(256), 0, s, t, out, n_out);
  return hipGetLastError();
}

}  // namespace ce
