// ce_opfile.hip -- the op-file writers' shared file size pass (gfx950, ce_opfile.h): the Orswot
// add-op and Rm-op writers' files are runs of ops whose byte lengths are already summed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ce_opfile_device.h"

namespace ce {
namespace {

// a lane per file: the data version, the Vec's header and its ops' bytes; the envelope's two bin
// headers at whatever form the length takes
__global__ __launch_bounds__(256) void k_opfile_sizes(OpFileLayout L, const uint32_t* ooff, uint32_t opf, uint32_t n_ops) {
  if (blockIdx.x == 0 && threadIdx.x == 0) L.clen[L.n_files] = L.xlen[L.n_files] = 0;
  for (uint32_t f = blockIdx.x * 256 + threadIdx.x; f < L.n_files; f += gridDim.x * 256) {
    const uint32_t j0 = f * opf, left = n_ops - j0, nops = left < opf ? left : opf;
    opfile_set_sizes(L, f, 16 + arr_hdr_len(nops) + (ooff[j0 + nops] - ooff[j0]));
  }
}

}  // namespace

hipError_t launch_opfile_sizes(hipStream_t s, const OpFileLayout& L, const uint32_t* ooff, uint32_t opf, uint32_t n_ops) {
  if (L.n_files == 0) return hipSuccess;
  hipLaunchKernelGGL(k_opfile_sizes, dim3(grid_blocks(L.n_files, 256, 4096)), dim3(256), 0, s, L, ooff, opf, n_ops);
  return hipGetLastError();
}

}  // namespace ce
