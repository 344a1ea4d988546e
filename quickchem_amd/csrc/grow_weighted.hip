// gfx950 kernels of boosting with row weights (grow.hpp GrowArgs; design in docs/21_row_weights.md).
//
//   grow_hist_weighted_kernel      once per level: grow_hist_kernel with a second fixed-point sum in place of the row
//                                  count - q = rint(g * w * 2^24) and hq = rint(w * 2^24) go into the block's LDS
//                                  histogram with two 64-bit integer adds a feature, 16 bytes a bin; the block flushes
//                                  the bins where either sum is nonzero with 64-bit global adds.
//   grow_split_weighted_kernel<0>  grow_split_kernel<0> with the fixed-point hessian policy (grow.hpp GrowFixedHess): its gain and
//                                  validity.
//   grow_split_weighted_kernel<1>  grow_split_kernel<1> with that policy: its leaf solve and the min_child_weight rule.
//   grow_sse_weighted_kernel       grow_sse_kernel with hq * e^2 in three 64-bit registers a lane; the launch for t = 0
//                                  also checks the weights and sums W.
//   grow_walk_sse_weighted_kernel  grow_walk_sse_kernel's walk, then the same sums.
// A row's weight, the three-part sums and their reduction are grow_sums_device.hpp's (grow_deep.hip walks with them too).
// The partition and leaf kernels read no weight and are grow.hip's own (launch_grow_partition, launch_grow_leaf).
// Only integer adds: no float atomics, no compare-and-swap loops, and the same trees and sums whatever the order of the
// rows or the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_device.hpp"
#include "grow_sums_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;
constexpr int kHistBlock = (int)kGrowHistBlock;

// grid (blocks over the rows, node groups x feature groups); dynamic LDS: node_group x feat_group x 256 x (8 + 8)
__global__ __launch_bounds__(kHistBlock) void grow_hist_weighted_kernel(GrowArgs a, uint32_t level, uint32_t node_group,
                                                                        uint32_t feat_group, uint32_t feat_groups) {
  extern __shared__ unsigned long long grow_whist[];
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  const uint32_t slot0 = (blockIdx.y / feat_groups) * node_group;
  const uint32_t f0 = (blockIdx.y % feat_groups) * feat_group;
  if (slot0 >= count || f0 >= a.num_feature) return;
  const uint32_t nslots = count - slot0 < node_group ? count - slot0 : node_group;
  const uint32_t nf = a.num_feature - f0 < feat_group ? a.num_feature - f0 : feat_group;
  const uint32_t cells = node_group * feat_group * kGrowBins;
  unsigned long long* Gl = grow_whist;
  unsigned long long* Hl = grow_whist + cells;
  for (uint32_t i = threadIdx.x; i < 2u * cells; i += kHistBlock) grow_whist[i] = 0ull;
  __syncthreads();
  const uint32_t first = begin + slot0;
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kHistBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kHistBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t s = (uint32_t)a.pos[row] - first;   // (a node below `first` wraps past nslots)
    if (s >= nslots) continue;
    const float g = a.pred[row] - a.labels[row];
    // the gradient before the weight (a NaN fails the comparison)
    if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) {
      flags |= kGrowFlagLabel;
      continue;
    }
    float w;
    unsigned long long hq;
    if (!grow_row_weight(a.weights, row, &w, &hq)) {
      flags |= kGrowFlagWeight;
      continue;
    }
    const float gw = g * w;   // one float32 multiply (-ffp-contract=off)
    if (!(__builtin_fabsf(gw) < kRefitMaxAbsGrad)) {
      flags |= kGrowFlagLabel;
      continue;
    }
    const unsigned long long q = (unsigned long long)(long long)__builtin_rintf(gw * kRefitGradScale);
    if (hq == 0ull && q == 0ull) continue;   // nothing to add
    const uint8_t* bin = a.bins + (uint64_t)f0 * a.nrow + row;
    const uint32_t base = s * feat_group * kGrowBins;
    for (uint32_t k = 0; k < nf; ++k) {
      const uint32_t i = base + k * kGrowBins + bin[(uint64_t)k * a.nrow];
      atomicAdd(&Gl[i], q);
      atomicAdd(&Hl[i], hq);
    }
  }
  if (flags) atomicOr(&a.state->error, flags);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < cells; i += kHistBlock) {
    const unsigned long long g = Gl[i], h = Hl[i];
    if ((g | h) == 0ull) continue;
    const uint32_t s = i / (feat_group * kGrowBins), k = (i / kGrowBins) % feat_group, b = i % kGrowBins;
    if (s >= nslots || k >= nf) continue;
    const uint64_t gi = ((uint64_t)(slot0 + s) * a.num_feature + f0 + k) * kGrowBins + b;
    if (h != 0ull) atomicAdd(&a.Hhist[gi], h);
    if (g != 0ull) atomicAdd(&a.Ghist[gi], g);
  }
}

// PHASE 0: grid (blocks of four waves over slots x features).  PHASE 1: one block.  The bodies are grow_device.hpp's,
// here with the fixed-point hessian sum and a histogram column for every feature.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void grow_split_weighted_kernel(GrowArgs a, uint32_t level, uint32_t round) {
  const GrowFixedHess hess{a.min_child_weight};
  if (PHASE == 0) {
    grow_split_columns(a, hess, level, round, a.num_feature, GrowIdentityMap());
  } else {
    grow_split_nodes<false>(a, hess, level, round, a.num_feature);
  }
}

// ---- the metric ----

// grid (blocks).  wslot: the set's W at t = 0, else nullptr
__global__ __launch_bounds__(kBlock) void grow_sse_weighted_kernel(GrowEvalArgs a, unsigned long long* slot,
                                                                   unsigned long long* wslot) {
  GrowWideAcc acc;
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    float w;
    unsigned long long hq;
    const bool sound = grow_row_weight(a.weights, row, &w, &hq);
    if (!grow_add_weighted_square(a.pred[row], a.labels[row], hq, &acc)) flags |= a.label_flag;
    if (!sound) flags |= a.weight_flag;
    acc.w += hq;
  }
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, wslot);
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_walk_sse_weighted_kernel(GrowEvalArgs a, uint32_t round, unsigned long long* slot) {
  __shared__ EvalNode tree[kGrowMaxNodes];
  const uint32_t count = grow_stage_tree(a, round, tree);
  if (count == 0) return;
  GrowWideAcc acc;
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
    float w;
    unsigned long long hq;
    if (!grow_row_weight(a.weights, row, &w, &hq)) flags |= a.weight_flag;
    if (!grow_add_weighted_square(pred, a.labels[row], hq, &acc)) flags |= a.label_flag;
  }
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, nullptr);
}

bool eval_args_sound(const GrowEvalArgs& a, uint32_t blocks, uint32_t set) {
  return a.nrow != 0 && a.nrow <= kRefitMaxRows && blocks != 0 && set <= 1 && a.pred != nullptr && a.labels != nullptr &&
         a.wsums != nullptr && a.state != nullptr &&
         ((a.label_flag == kGrowFlagLabel && a.weight_flag == kGrowFlagWeight) ||
          (a.label_flag == kGrowFlagEvalLabel && a.weight_flag == kGrowFlagEvalWeight));
}

}  // namespace

int grow_lds_limits_weighted() {
  return raise_lds_limit(grow_hist_weighted_kernel, kGrowWeightedMaxPairs * kGrowWeightedPairBytes);
}

namespace {

hipError_t weighted_levels(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, hipStream_t stream,
                           bool leaf) {
  if (!(a.min_child_weight >= 0.0)) return hipErrorInvalidValue;
  return grow_launch_tree(
      a, plan, levels, round, stream, a.num_feature, kGrowWeightedPairBytes, 0,
      [&](const GrowLevelPlan& l, uint32_t d) {
        hipLaunchKernelGGL(grow_hist_weighted_kernel, dim3(l.hist_blocks, l.node_groups * l.feat_groups), dim3(kHistBlock),
                           l.lds_bytes, stream, a, d, l.node_group, l.feat_group, l.feat_groups);
      },
      [&](uint32_t blocks, uint32_t d) {
        hipLaunchKernelGGL(grow_split_weighted_kernel<0>, dim3(blocks), dim3(kBlock), 0, stream, a, d, round);
      },
      [&](uint32_t d) { hipLaunchKernelGGL(grow_split_weighted_kernel<1>, dim3(1), dim3(kBlock), 0, stream, a, d, round); }, leaf);
}

}  // namespace

int launch_grow_tree_weighted(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream) {
  return weighted_levels(a, plan, levels, round, static_cast<hipStream_t>(stream), true);
}

int launch_grow_levels_weighted(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream) {
  return weighted_levels(a, plan, levels, round, static_cast<hipStream_t>(stream), false);
}

int launch_grow_sse_weighted(const GrowEvalArgs& a, uint32_t blocks, uint32_t t, uint32_t set, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!eval_args_sound(a, blocks, set)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_sse_weighted_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, a.wsums + grow_wide_index(t, set),
                     t == 0 ? a.wsums + set : nullptr);
  return hipGetLastError();
}

int launch_grow_walk_sse_weighted(const GrowEvalArgs& a, uint32_t blocks, uint32_t round, uint32_t set, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!eval_args_sound(a, blocks, set) || a.bins == nullptr || a.nodes == nullptr || a.tree_nodes == nullptr ||
      a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 || a.max_depth > kGrowMaxDepth)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_walk_sse_weighted_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, round,
                     a.wsums + grow_wide_index(round + 1, set));
  return hipGetLastError();
}

}  // namespace ohx
