// gfx950 kernels of the tree grower (grow.hpp; design in docs/18_boost_trees.md).
//
//   grow_bin_kernel        once per call: the cuts are staged in LDS, a lane takes a row and finds each value's bin by
//                          binary search; bins[f][row] is feature-major, so a wave's 64 bins are 64 contiguous bytes.
//   grow_hist_kernel       once per level: a lane takes a row, recomputes q from pred and the label, and adds it into
//                          the block's LDS histogram of its (node group, feature group) with a 64-bit integer add, the
//                          row count with a 32-bit one; the block flushes its nonzero bins once with 64-bit global adds.
//   grow_split_kernel<0>   once per level: a wave per (node, feature) - integer prefix sums across the 256 bins, the
//                          shared gain in double, and a butterfly reduction by the total order of grow_better.
//   grow_split_kernel<1>   once per level, one block: a thread per open node takes the best of its features, the
//                          splitting nodes get their child ids in ascending node order, the records are written.
//   grow_partition_kernel  once per level: a row on a node that split steps to the child its bin says.
//   grow_leaf_kernel       once per tree: pred += leaf[pos], pos = 0.
// Only integer adds: no float atomics, no compare-and-swap loops, and the same trees whatever the order of the rows or
// the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;
constexpr int kHistBlock = (int)kGrowHistBlock;

// grid (blocks); dynamic LDS: the cuts
__global__ __launch_bounds__(kBlock) void grow_bin_kernel(GrowArgs a) {
  extern __shared__ float grow_cuts[];
  for (uint32_t i = threadIdx.x; i < a.ncuts; i += kBlock) grow_cuts[i] = a.cuts[i];
  __syncthreads();
  const bool missing_is_nan = a.missing != a.missing;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const float* x = a.rows + row * (uint64_t)a.ncol;
    for (uint32_t f = 0; f < a.num_feature; ++f) {
      const uint32_t c0 = a.cut_ptr[f], c1 = a.cut_ptr[f + 1];
      uint32_t b = kGrowMissingBin;
      if (f < a.ncol) {
        const float v = x[f];
        if (!(v != v || (!missing_is_nan && v == a.missing))) {
          // b = #{j : c_j <= v}
          uint32_t lo = c0, hi = c1;
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (grow_cuts[mid] <= v) lo = mid + 1;
            else hi = mid;
          }
          b = lo - c0;
        }
      }
      a.bins[(uint64_t)f * a.nrow + row] = (uint8_t)b;
    }
  }
}

// grid (blocks over the rows, node groups x feature groups); dynamic LDS: node_group x feat_group x 256 x (8 + 4)
__global__ __launch_bounds__(kHistBlock) void grow_hist_kernel(GrowArgs a, uint32_t level, uint32_t node_group,
                                                               uint32_t feat_group, uint32_t feat_groups) {
  extern __shared__ unsigned long long grow_hist[];
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  const uint32_t slot0 = (blockIdx.y / feat_groups) * node_group;
  const uint32_t f0 = (blockIdx.y % feat_groups) * feat_group;
  if (slot0 >= count || f0 >= a.num_feature) return;
  const uint32_t nslots = count - slot0 < node_group ? count - slot0 : node_group;
  const uint32_t nf = a.num_feature - f0 < feat_group ? a.num_feature - f0 : feat_group;
  const uint32_t cells = node_group * feat_group * kGrowBins;
  unsigned long long* Gl = grow_hist;
  uint32_t* Hl = reinterpret_cast<uint32_t*>(grow_hist + cells);
  for (uint32_t i = threadIdx.x; i < cells; i += kHistBlock) {
    Gl[i] = 0ull;
    Hl[i] = 0u;
  }
  __syncthreads();
  const uint32_t first = begin + slot0;
  const uint64_t stride = (uint64_t)gridDim.x * kHistBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kHistBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t s = (uint32_t)a.pos[row] - first;   // (a node below `first` wraps past nslots)
    if (s >= nslots) continue;
    const float g = a.pred[row] - a.labels[row];
    // (a NaN fails the comparison)
    if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) {
      atomicOr(&a.state->error, kGrowFlagLabel);
      continue;
    }
    const unsigned long long q = (unsigned long long)(long long)__builtin_rintf(g * kRefitGradScale);
    const uint8_t* bin = a.bins + (uint64_t)f0 * a.nrow + row;
    const uint32_t base = s * feat_group * kGrowBins;
    for (uint32_t k = 0; k < nf; ++k) {
      const uint32_t i = base + k * kGrowBins + bin[(uint64_t)k * a.nrow];
      atomicAdd(&Gl[i], q);
      atomicAdd(&Hl[i], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < cells; i += kHistBlock) {
    const uint32_t h = Hl[i];
    if (h == 0u) continue;
    const uint32_t s = i / (feat_group * kGrowBins), k = (i / kGrowBins) % feat_group, b = i % kGrowBins;
    if (s >= nslots || k >= nf) continue;
    const uint64_t gi = ((uint64_t)(slot0 + s) * a.num_feature + f0 + k) * kGrowBins + b;
    atomicAdd(&a.Hhist[gi], (unsigned long long)h);
    const unsigned long long g = Gl[i];
    if (g != 0ull) atomicAdd(&a.Ghist[gi], g);
  }
}

// PHASE 0: grid (blocks of four waves over slots x features).  PHASE 1: one block.  The bodies are grow_device.hpp's,
// here with a row count for a hessian sum and a histogram column for every feature.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void grow_split_kernel(GrowArgs a, uint32_t level, uint32_t round) {
  const GrowCountHess hess{a.min_child_rows};
  if (PHASE == 0) {
    grow_split_columns(a, hess, level, round, a.num_feature, GrowIdentityMap());
  } else {
    grow_split_nodes<false>(a, hess, level, round, a.num_feature);
  }
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_partition_kernel(GrowArgs a, uint32_t round) {
  const GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const uint32_t next = a.state->next;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t p = a.pos[row];
    if (p >= next) {
      atomicOr(&a.state->error, kGrowFlagState);
      continue;
    }
    const int32_t left = nodes[p].left;
    if (left < 0) continue;
    const uint32_t f = nodes[p].feature;
    if (f >= a.num_feature) {
      atomicOr(&a.state->error, kGrowFlagState);
      continue;
    }
    const uint32_t b = a.bins[(uint64_t)f * a.nrow + row];
    const bool go_left = b == kGrowMissingBin ? nodes[p].default_left != 0u : b <= nodes[p].cut;
    a.pos[row] = (uint16_t)(go_left ? left : nodes[p].right);
  }
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_leaf_kernel(GrowArgs a, uint32_t round) {
  const GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const uint32_t next = a.state->next;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t p = a.pos[row];
    if (p < next) a.pred[row] += nodes[p].value;
    else atomicOr(&a.state->error, kGrowFlagState);
    a.pos[row] = 0;
  }
}

}  // namespace

int grow_lds_limits() {
  hipError_t e = raise_lds_limit(grow_bin_kernel, kGrowMaxFeatures * kGrowMaxCuts * sizeof(float));
  if (e != hipSuccess) return e;
  return raise_lds_limit(grow_hist_kernel, kGrowMaxPairs * kGrowPairBytes);
}

int launch_grow_bin(const GrowArgs& a, const GrowPlan& plan, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || a.ncol > a.num_feature || a.num_feature == 0 ||
      a.num_feature > kGrowMaxFeatures || (uint64_t)a.ncuts > (uint64_t)a.num_feature * kGrowMaxCuts ||
      plan.bin_lds_bytes != a.ncuts * sizeof(float) || plan.row_blocks == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_bin_kernel, dim3(plan.row_blocks), dim3(kBlock), plan.bin_lds_bytes, stream, a);
  return hipGetLastError();
}

int launch_grow_tree(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (a.min_child_rows < 1) return hipErrorInvalidValue;
  // (kGrowMaxTrips: this histogram kernel alone counts a bin's rows in 32 bits of LDS)
  return grow_launch_tree(
      a, plan, levels, round, stream, a.num_feature, kGrowPairBytes, kGrowMaxTrips,
      [&](const GrowLevelPlan& l, uint32_t d) {
        hipLaunchKernelGGL(grow_hist_kernel, dim3(l.hist_blocks, l.node_groups * l.feat_groups), dim3(kHistBlock), l.lds_bytes,
                           stream, a, d, l.node_group, l.feat_group, l.feat_groups);
      },
      [&](uint32_t blocks, uint32_t d) { hipLaunchKernelGGL(grow_split_kernel<0>, dim3(blocks), dim3(kBlock), 0, stream, a, d, round); },
      [&](uint32_t d) { hipLaunchKernelGGL(grow_split_kernel<1>, dim3(1), dim3(kBlock), 0, stream, a, d, round); });
}

int launch_grow_partition(const GrowArgs& a, const GrowPlan& plan, uint32_t round, void* stream_) {
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || plan.row_blocks == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_partition_kernel, dim3(plan.row_blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream_), a, round);
  return hipGetLastError();
}

int launch_grow_leaf(const GrowArgs& a, const GrowPlan& plan, uint32_t round, void* stream_) {
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || plan.row_blocks == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_leaf_kernel, dim3(plan.row_blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream_), a, round);
  return hipGetLastError();
}

}  // namespace ohx
