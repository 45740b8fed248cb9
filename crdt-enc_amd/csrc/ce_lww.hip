// ce_lww.hip -- LWWReg<u64, u64> on the device (gfx950): the wave-per-file decode of an op file's
// Vec<LWWReg> from plaintext in HBM (multi-page files, host-parse envelopes, multi-key retries)
// and the reduce of the per-file records (ce_lww.h) to the batch's winner (k_lww_reduce by file
// index; k_lww_reduce_keyed by the files' addresses, for a share of a batch partitioned across ranks).
//
// Element grammar: parse_lww_op (ce_lww.h).  The form rmp-serde's to_vec_named writes is
//   82 a3"val" <uint> a6"marker" <uint>      12 + wv + wm bytes, wv, wm in {1, 2, 3, 5, 9}
// and a file whose elements all have the first one's (wv, wm) is read at a fixed stride.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_lww.h"

namespace ce {
namespace {

constexpr int kWaves = 4;  // waves per block

// (marker, index) order of the fold: a beats b when its marker is larger, or equal and earlier
__device__ __forceinline__ bool lww_better(unsigned long long ma, uint32_t ia, unsigned long long mb, uint32_t ib) {
  return ma > mb || (ma == mb && ia < ib);
}

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
  return ((unsigned long long)hi << 32) | lo;
}

// the wave's best (marker, idx, val) into every lane
__device__ __forceinline__ void wave_best(unsigned long long& m, uint32_t& i, unsigned long long& v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long om = shfl_xor64(m, d), ov = shfl_xor64(v, d);
    const uint32_t oi = (uint32_t)__shfl_xor((int)i, d);
    if (lww_better(om, oi, m, i)) { m = om; i = oi; v = ov; }
  }
}

// the uint of w bytes (marker included) at p[0..w), big-endian payload
__device__ __forceinline__ unsigned long long lww_uint(const uint8_t* p, uint32_t w) {
  if (w == 1) return p[0];
  unsigned long long x = 0;
  for (uint32_t k = 1; k < w; k++) x = (x << 8) | p[k];
  return x;
}

// the element at e[0 .. 12 + wv + wm), all of it inside the file: true when it is the written
// form with these widths
__device__ bool lww_elem_fixed(const uint8_t* e, uint32_t wv, uint32_t wm, unsigned long long* val,
                               unsigned long long* marker) {
  if (e[0] != 0x82 || e[1] != 0xa3 || e[2] != 'v' || e[3] != 'a' || e[4] != 'l') return false;
  if (lww_uint_width(e[5]) != wv) return false;
  const uint8_t* k = e + 5 + wv;
  if (k[0] != 0xa6 || k[1] != 'm' || k[2] != 'a' || k[3] != 'r' || k[4] != 'k' || k[5] != 'e' || k[6] != 'r')
    return false;
  if (lww_uint_width(k[7]) != wm) return false;
  *val = lww_uint(e + 5, wv);
  *marker = lww_uint(k + 7, wm);
  return true;
}

__device__ void decode_lww_file(const LwwDecodeArgs& a, uint32_t f, uint32_t lane) {
  const FileParams* Pp = a.params + f;
  const uint8_t* pt = a.pt + Pp->out_off;
  const uint32_t len = Pp->len;
  int32_t st = CE_OK;
  // clear text = VersionBytes(data_version, msgpack(Vec<LWWReg>)) (crdt-enc/src/lib.rs:504-507)
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
  unsigned long long bm = 0, bv = 0;  // the file's winner: marker 0 never wins
  uint32_t bi = 0xffffffffu;
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
      // uniform stride: the first element's two integer markers give (wv, wm), and count x stride
      // fits, so every element lies whole inside the file.  Lane L checks elements L, L + 64, ...
      // whole and keeps its best, replacing on strictly greater only (its elements come in order)
      uint32_t wv = 0, wm = 0, stride = 0;
      if (cnt > 0 && blen - h >= 14) {
        wv = lww_uint_width(body[h + 5]);
        if (wv && h + 12 + wv < blen) wm = lww_uint_width(body[h + 12 + wv]);
        if (wv && wm) stride = 12 + wv + wm;
        if (stride && (unsigned long long)cnt * stride > blen - h) stride = 0;
      }
      bool ok = stride != 0;
      if (stride)
        for (uint32_t e = lane; e < cnt && ok; e += 64) {
          unsigned long long v, m;
          ok = lww_elem_fixed(body + h + (unsigned long long)e * stride, wv, wm, &v, &m);
          if (ok && m > bm) { bm = m; bv = v; bi = e; }
        }
      const bool uniform = cnt == 0 || __ballot(ok) == ~0ull;
      if (uniform) {
        if (lane == 0) atomicAdd(&a.paths[0], 1u);
        wave_best(bm, bi, bv);
      } else {
        // general: lane 0 walks the elements front to back through the host's parser
        if (lane == 0) {
          atomicAdd(&a.paths[1], 1u);
          bm = 0;
          bv = 0;
          Rd q{body, blen, h};
          for (uint32_t e = 0; e < cnt; e++) {
            uint64_t v = 0, m = 0;
            if (parse_lww_op(q, &v, &m) != 1) { st = CE_ERR_DECODE; break; }  // (too deep: rejected)
            if (m > bm) { bm = m; bv = v; }
          }
        }
      }
    }
  }
  if (lane == 0) {
    atomicAdd(&a.paths[3], 1u);
    if (st != CE_OK) a.status[f] = st;
    // (a multi-key retry decodes a file whose row an earlier pass may have left: written either way)
    const bool win = st == CE_OK && a.apply[f] && bm != 0;
    a.rec[f] = LwwRec{win ? bm : 0ull, win ? bv : 0ull};
  }
}

__global__ __launch_bounds__(256) void k_decode_lww(LwwDecodeArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t stride = gridDim.x * kWaves;
  for (uint32_t f = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6)); f < a.n; f += stride) {
    if (a.only && !a.only[f]) continue;
    if (a.large_only && a.params[f].len <= kSmallMax) continue;  // (the fused open decoded those)
    if (a.status[f] != CE_OK) continue;
    decode_lww_file(a, f, lane);
  }
}

// the block's best of (m, i, v) into thread 0
__device__ __forceinline__ void block_best(unsigned long long& m, uint32_t& i, unsigned long long& v) {
  __shared__ unsigned long long s_m[kLwwBlock / 64], s_v[kLwwBlock / 64];
  __shared__ uint32_t s_i[kLwwBlock / 64];
  wave_best(m, i, v);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_m[w] = m; s_v[w] = v; s_i[w] = i; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t k = 1; k < kLwwBlock / 64; k++)
      if (lww_better(s_m[k], s_i[k], m, i)) { m = s_m[k]; i = s_i[k]; v = s_v[k]; }
}

// stage 1: block b takes tiles b, b + grid, ... of kLwwTile records and leaves part[b]
__global__ __launch_bounds__(kLwwBlock) void k_lww_reduce(const LwwRec* rec, uint32_t n, LwwPartial* part) {
  static_assert(kLwwTile % kLwwBlock == 0, "a tile is whole rounds of the block");
  unsigned long long bm = 0, bv = 0;
  uint32_t bi = 0xffffffffu;
  const uint32_t tiles = (uint32_t)(((unsigned long long)n + kLwwTile - 1) / kLwwTile);
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    // (t < tiles: t * kLwwTile < n; the indices below are computed in 64 bits)
    const unsigned long long base = (unsigned long long)t * kLwwTile;
#pragma unroll
    for (uint32_t r = 0; r < kLwwTile / kLwwBlock; r++) {
      const unsigned long long i = base + r * kLwwBlock + threadIdx.x;
      if (i < n) {
        const LwwRec x = rec[i];
        if (lww_better(x.marker, (uint32_t)i, bm, bi)) { bm = x.marker; bv = x.val; bi = (uint32_t)i; }
      }
    }
  }
  block_best(bm, bi, bv);
  if (threadIdx.x == 0) part[blockIdx.x] = LwwPartial{bm, bv, bi, 0};
}

// the final stage: one block over the k <= kLwwMaxBlocks partials
__global__ __launch_bounds__(kLwwBlock) void k_lww_reduce_final(const LwwPartial* part, uint32_t k, LwwRec* out) {
  unsigned long long bm = 0, bv = 0;
  uint32_t bi = 0xffffffffu;
  for (uint32_t j = threadIdx.x; j < k; j += kLwwBlock) {
    const LwwPartial p = part[j];
    if (lww_better(p.marker, p.idx, bm, bi)) { bm = p.marker; bv = p.val; bi = p.idx; }
  }
  block_best(bm, bi, bv);
  if (threadIdx.x == 0) out[0] = LwwRec{bm, bm ? bv : 0ull};
}

// ---- the keyed reduce: the same two stages, each candidate carried with its address ----
struct Keyed {
  unsigned long long m, v, fv;
  uint32_t fa, i;
};

__device__ __forceinline__ bool keyed_better(const Keyed& a, const Keyed& b) {
  return lww_keyed_better(a.m, a.fa, a.fv, a.i, b.m, b.fa, b.fv, b.i);
}

// the wave's best into every lane
__device__ __forceinline__ void wave_best_keyed(Keyed& x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    Keyed o;
    o.m = shfl_xor64(x.m, d);
    o.v = shfl_xor64(x.v, d);
    o.fv = shfl_xor64(x.fv, d);
    o.fa = (uint32_t)__shfl_xor((int)x.fa, d);
    o.i = (uint32_t)__shfl_xor((int)x.i, d);
    if (keyed_better(o, x)) x = o;
  }
}

// the block's best into thread 0
__device__ __forceinline__ void block_best_keyed(Keyed& x) {
  __shared__ Keyed s_k[kLwwBlock / 64];
  wave_best_keyed(x);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_k[w] = x;
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t k = 1; k < kLwwBlock / 64; k++)
      if (keyed_better(s_k[k], x)) x = s_k[k];
}

// stage 1: as k_lww_reduce, record i read with fa[i] / fv[i]
__global__ __launch_bounds__(kLwwBlock) void k_lww_reduce_keyed(const LwwRec* rec, const uint32_t* fa,
                                                                const uint64_t* fv, uint32_t n,
                                                                LwwKeyedPartial* part) {
  Keyed b{0ull, 0ull, ~0ull, 0xffffffffu, 0xffffffffu};
  const uint32_t tiles = (uint32_t)(((unsigned long long)n + kLwwTile - 1) / kLwwTile);
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    // (t < tiles: t * kLwwTile < n; the indices below are computed in 64 bits)
    const unsigned long long base = (unsigned long long)t * kLwwTile;
#pragma unroll
    for (uint32_t r = 0; r < kLwwTile / kLwwBlock; r++) {
      const unsigned long long i = base + r * kLwwBlock + threadIdx.x;
      if (i < n) {
        const LwwRec x = rec[i];
        const Keyed c{x.marker, x.val, fv[i], fa[i], (uint32_t)i};
        if (keyed_better(c, b)) b = c;
      }
    }
  }
  block_best_keyed(b);
  if (threadIdx.x == 0) part[blockIdx.x] = LwwKeyedPartial{b.m, b.v, b.fv, b.fa, b.i};
}

// the final stage: one block over the k <= kLwwMaxBlocks partials
__global__ __launch_bounds__(kLwwBlock) void k_lww_reduce_keyed_final(const LwwKeyedPartial* part, uint32_t k,
                                                                      LwwKeyed* out) {
  Keyed b{0ull, 0ull, ~0ull, 0xffffffffu, 0xffffffffu};
  for (uint32_t j = threadIdx.x; j < k; j += kLwwBlock) {
    const LwwKeyedPartial p = part[j];
    const Keyed c{p.marker, p.val, p.fv, p.fa, p.idx};
    if (keyed_better(c, b)) b = c;
  }
  block_best_keyed(b);
  if (threadIdx.x == 0)
    out[0] = b.m ? LwwKeyed{b.m, b.v, (unsigned long long)b.fa, b.fv} : LwwKeyed{0ull, 0ull, ~0ull, ~0ull};
}

}  // namespace

hipError_t launch_decode_lww(hipStream_t s, const LwwDecodeArgs& a, uint32_t grid_waves) {
  if (a.n == 0) return hipSuccess;
  const uint32_t blocks = (grid_waves + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(k_decode_lww, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_lww_reduce(hipStream_t s, const LwwRec* rec, uint32_t n, LwwPartial* part, LwwRec* out,
                             uint32_t grid_cap) {
  if (n == 0) return hipErrorInvalidValue;
  const uint32_t tiles = (uint32_t)(((uint64_t)n + kLwwTile - 1) / kLwwTile);
  uint32_t blocks = tiles < kLwwMaxBlocks ? tiles : kLwwMaxBlocks;
  if (grid_cap && blocks > grid_cap) blocks = grid_cap;
  hipLaunchKernelGGL(k_lww_reduce, dim3(blocks), dim3(kLwwBlock), 0, s, rec, n, part);
  hipLaunchKernelGGL(k_lww_reduce_final, dim3(1), dim3(kLwwBlock), 0, s, part, blocks, out);
  return hipGetLastError();
}

hipError_t launch_lww_reduce_keyed(hipStream_t s, const LwwRec* rec, const uint32_t* fa, const uint64_t* fv,
                                   uint32_t n, LwwKeyedPartial* part, LwwKeyed* out, uint32_t grid_cap) {
  if (n == 0) return hipErrorInvalidValue;
  const uint32_t tiles = (uint32_t)(((uint64_t)n + kLwwTile - 1) / kLwwTile);
  uint32_t blocks = tiles < kLwwMaxBlocks ? tiles : kLwwMaxBlocks;
  if (grid_cap && blocks > grid_cap) blocks = grid_cap;
  hipLaunchKernelGGL(k_lww_reduce_keyed, dim3(blocks), dim3(kLwwBlock), 0, s, rec, fa, fv, n, part);
  hipLaunchKernelGGL(k_lww_reduce_keyed_final, dim3(1), dim3(kLwwBlock), 0, s, part, blocks, out);
  return hipGetLastError();
}

}  // namespace ce
