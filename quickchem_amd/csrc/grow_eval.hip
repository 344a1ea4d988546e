// gfx950 kernels of the held-out metric (grow.hpp GrowEvalArgs; design in docs/20_boost_eval.md).
//
//   grow_sse_kernel        any rows: a lane takes a row, q = rint((pred - label) * 2^24) as the histogram kernel makes it,
//                          and adds the high and the low 32 bits of q^2 to two 64-bit registers; waves are reduced with
//                          shuffles, the block through LDS, and one pair of 64-bit global integer adds leaves a block.
//   grow_walk_sse_kernel   the held-out rows, once per new tree: the block stages the tree's records in LDS (16 bytes a
//                          node), a lane walks its row from the root by the bin planes as grow_partition_kernel steps,
//                          pred += leaf, then the same residual, square and reduction.
// Only integer adds: the sums depend on neither the order of the rows nor the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;
constexpr int kWaves = kBlock / kWave;

// one row's square into the lane's accumulators; false where the residual is out of range
__device__ inline bool add_square(float pred, float label, unsigned long long* hi, unsigned long long* lo) {
  const float g = pred - label;
  // (a NaN fails the comparison)
  if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) return false;
  const long long q = (long long)__builtin_rintf(g * kRefitGradScale);
  const unsigned long long a = (unsigned long long)(q < 0 ? -q : q);   // <= 2^32 - 256
  const unsigned long long s = a * a;
  *hi += s >> 32;
  *lo += s & 0xFFFFFFFFull;
  return true;
}

// the block's two sums leave it with one pair of global adds
__device__ inline void reduce_and_add(unsigned long long hi, unsigned long long lo, unsigned long long* slot) {
  __shared__ unsigned long long part[kWaves][2];
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    hi += __shfl_xor(hi, d, kWave);
    lo += __shfl_xor(lo, d, kWave);
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    part[wave][0] = hi;
    part[wave][1] = lo;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long h = 0, l = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      h += part[w][0];
      l += part[w][1];
    }
    atomicAdd(&slot[0], h);
    atomicAdd(&slot[1], l);
  }
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_sse_kernel(GrowEvalArgs a, unsigned long long* slot) {
  unsigned long long hi = 0, lo = 0;
  bool bad = false;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride)
    bad |= !add_square(a.pred[row], a.labels[row], &hi, &lo);
  if (bad) atomicOr(&a.state->error, a.label_flag);
  reduce_and_add(hi, lo, slot);
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_walk_sse_kernel(GrowEvalArgs a, uint32_t round, unsigned long long* slot) {
  __shared__ EvalNode tree[kGrowMaxNodes];
  const uint32_t count = grow_stage_tree(a, round, tree);
  if (count == 0) return;
  unsigned long long hi = 0, lo = 0;
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    uint32_t leaf;
    if (!grow_walk_row(a, tree, count, row, &leaf)) {
      flags |= kGrowFlagState;
      continue;
    }
    const float pred = a.pred[row] + tree[leaf].value;
    a.pred[row] = pred;
    if (!add_square(pred, a.labels[row], &hi, &lo)) flags |= a.label_flag;
  }
  if (flags) atomicOr(&a.state->error, flags);
  reduce_and_add(hi, lo, slot);
}

bool args_sound(const GrowEvalArgs& a, uint32_t blocks) {
  return a.nrow != 0 && a.nrow <= kRefitMaxRows && blocks != 0 && a.pred != nullptr && a.labels != nullptr &&
         a.sums != nullptr && a.state != nullptr && (a.label_flag == kGrowFlagLabel || a.label_flag == kGrowFlagEvalLabel);
}

}  // namespace

int launch_grow_sse(const GrowEvalArgs& a, uint32_t blocks, uint32_t t, uint32_t set, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!args_sound(a, blocks) || set > 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_sse_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, a.sums + grow_sum_index(t, set));
  return hipGetLastError();
}

int launch_grow_walk_sse(const GrowEvalArgs& a, uint32_t blocks, uint32_t round, uint32_t set, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!args_sound(a, blocks) || set > 1 || a.bins == nullptr || a.nodes == nullptr || a.tree_nodes == nullptr ||
      a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 || a.max_depth > kGrowMaxDepth)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_walk_sse_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, round,
                     a.sums + grow_sum_index(round + 1, set));
  return hipGetLastError();
}

}  // namespace ohx
