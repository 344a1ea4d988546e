// gfx950 kernels of boosters with several output groups (groups.hpp; design in docs/13_output_groups.md).  Nothing here
// walks a tree: these kernels read what the walks and the contributions kernels wrote, one group plane or block at a
// time, and put it where xgboost 1.6.0's layouts want it.  Plain loads and stores, no atomics, no LDS.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "groups.hpp"

namespace ohx {

namespace {

constexpr int kBlock = 256;
// grid-stride kernels: at most this many blocks (8 waves a CU on 256 CUs), whatever the size
constexpr uint64_t kMaxBlocks = 2048;

unsigned blocks_for(uint64_t n) {
  const uint64_t b = (n + kBlock - 1) / kBlock;
  return (unsigned)(b < kMaxBlocks ? (b ? b : 1) : kMaxBlocks);
}

// One lane per row.  Lane r reads planes[g * nrow + r]: for every g the wave's loads are 64 consecutive floats.
__global__ __launch_bounds__(kBlock) void group_finish_kernel(const float* __restrict__ planes, uint64_t nrow,
                                                              uint32_t G, int mode, float* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < nrow; r += stride) {
    const float* x = planes + r;
    if (mode == kGroupMargins) {
      for (uint32_t g = 0; g < G; ++g) out[r * G + g] = x[(uint64_t)g * nrow];
    } else if (mode == kGroupArgmax) {
      float best = x[0];
      uint32_t idx = 0;
      for (uint32_t g = 1; g < G; ++g) {
        const float v = x[(uint64_t)g * nrow];
        if (best < v) {
          best = v;
          idx = g;
        }
      }
      out[r] = (float)idx;
    } else {
      float wmax = x[0];
      for (uint32_t g = 1; g < G; ++g) wmax = fmaxf(x[(uint64_t)g * nrow], wmax);
      double wsum = 0.0;
      for (uint32_t g = 0; g < G; ++g) wsum += (double)expf(x[(uint64_t)g * nrow] - wmax);
      const float div = (float)wsum;
      // expf of the same float again: the same e_g as the sum took
      for (uint32_t g = 0; g < G; ++g) out[r * G + g] = expf(x[(uint64_t)g * nrow] - wmax) / div;
    }
  }
}

__global__ __launch_bounds__(kBlock) void group_leaf_gather_kernel(const float* __restrict__ src, uint64_t nrow,
                                                                   uint32_t T, const uint32_t* __restrict__ flat_of_file,
                                                                   uint32_t L, float* __restrict__ out) {
  const uint64_t n = nrow * L, stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint64_t r = i / L;
    const uint32_t j = (uint32_t)(i - r * L);
    out[i] = src[r * T + flat_of_file[j]];
  }
}

__global__ __launch_bounds__(kBlock) void group_block_scatter_kernel(const float* __restrict__ src, uint64_t nrow,
                                                                     uint32_t W, uint32_t G, uint32_t g,
                                                                     float* __restrict__ out) {
  const uint64_t n = nrow * W, stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint64_t r = i / W;
    const uint64_t k = i - r * W;
    out[(r * G + g) * W + k] = src[i];
  }
}

}  // namespace

hipError_t launch_group_finish(const float* planes, uint64_t nrow, uint32_t G, int mode, float* out, hipStream_t stream) {
  if (nrow == 0 || G == 0) return hipSuccess;
  if (mode != kGroupMargins && mode != kGroupSoftprob && mode != kGroupArgmax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(group_finish_kernel, dim3(blocks_for(nrow)), dim3(kBlock), 0, stream, planes, nrow, G, mode, out);
  return hipGetLastError();
}

hipError_t launch_group_leaf_gather(const float* src, uint64_t nrow, uint32_t T, const uint32_t* flat_of_file,
                                    uint32_t L, float* out, hipStream_t stream) {
  if (nrow == 0 || L == 0) return hipSuccess;
  if (L > T) return hipErrorInvalidValue;
  hipLaunchKernelGGL(group_leaf_gather_kernel, dim3(blocks_for(nrow * L)), dim3(kBlock), 0, stream, src, nrow, T,
                     flat_of_file, L, out);
  return hipGetLastError();
}

hipError_t launch_group_block_scatter(const float* src, uint64_t nrow, uint32_t W, uint32_t G, uint32_t g, float* out,
                                      hipStream_t stream) {
  if (nrow == 0 || W == 0) return hipSuccess;
  if (g >= G) return hipErrorInvalidValue;
  hipLaunchKernelGGL(group_block_scatter_kernel, dim3(blocks_for(nrow * W)), dim3(kBlock), 0, stream, src, nrow, W, G,
                     g, out);
  return hipGetLastError();
}

}  // namespace ohx
