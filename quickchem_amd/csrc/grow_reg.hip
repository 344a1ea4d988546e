// gfx950 kernels of regularised boosting and of the metrics beside the RMSE (grow.hpp GrowRegHess, grow_metric_row; design
// in docs/27_regularisation_and_metrics.md).  A call runs them only where "ohx_reg_alpha", "ohx_max_delta_step" or
// "ohx_eval_metric" is set away from its default: with the defaults nothing of this file is touched, its code object
// included.
//
//   grow_split_reg_kernel<0, ..>        levels 0 - 7: grow_device.hpp's phase 0 with the regularised hessian policy over
//                                       a feature list (the pair path's columns).  The gain divides in double.
//   grow_split_reg_kernel<1, ROOT>      its phase 1: the regularised leaf solve.  ROOT is grow_split_pairs_kernel's.
//   grow_deep_split_reg_kernel<0>       levels 8 - 17, once per batch: grow_split_columns over the batch's histograms.
//   grow_deep_split_reg_kernel<1>       once per level, one block: grow_deep_device.hpp's chunked walk with the policy.
//   grow_sse_metric_kernel<M>           grow_sse_weighted_kernel with the row's term of metric M in place of e^2.
//   grow_walk_sse_metric_kernel<M>      grow_walk_sse_weighted_kernel likewise: the tree staged in LDS, at most 512 nodes.
//   grow_deep_walk_sse_metric_kernel<M> grow_deep_walk_sse_kernel likewise: the node table in HBM.
// The pair kernel, both pair histogram kernels, and the bin, partition, leaf, widen and stage kernels are the other
// files' own.  The metric kernels read the 12 bytes a row that the weighted ones read, raise the same flags and leave the
// block through grow_reduce_wide: integer global adds, no float atomics, no compare-and-swap loops, and the same sums
// whatever the order of the rows or the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_deep_device.hpp"
#include "grow_device.hpp"
#include "grow_sums_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;

// the histogram columns of the tree at hand: column k is feature list[k]
struct RegColumns {
  const uint8_t* list;
  uint32_t ncols;
};

// PHASE 0: grid (blocks of four waves over slots x columns).  PHASE 1: one block.
template <int PHASE, int ROOT>
__global__ __launch_bounds__(kBlock) void grow_split_reg_kernel(GrowArgs a, RegColumns c, GrowRegHess hess, uint32_t level,
                                                                uint32_t round) {
  if (PHASE == 0) {
    GrowListMap map;
    map.list = c.list;
    grow_split_columns(a, hess, level, round, c.ncols, map);
  } else {
    grow_split_nodes<ROOT == kGrowRootBag>(a, hess, level, round, c.ncols);
    // the root's sums are phase 0's, written before this kernel started
    if (ROOT == kGrowRootHess && level == 0 && threadIdx.x == 0 && a.nodes[(uint64_t)round * kGrowMaxNodes].H == 0)
      atomicOr(&a.state->error, kGrowFlagHess);
  }
}

// PHASE 0: grid (blocks of four waves over the batch's slots x columns).  PHASE 1: one block.  With d.g.features the
// columns are the tree's list, else every feature.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void grow_deep_split_reg_kernel(GrowDeepArgs d, GrowRegHess hess, uint32_t level,
                                                                     uint32_t round, uint32_t batch0) {
  const GrowArgs a = grow_deep_tree_args(d, round);
  const bool listed = a.features != nullptr;
  const uint32_t ncols = listed ? a.n_sel : a.num_feature;
  if (PHASE == 0) {
    if (listed) {
      GrowListMap map;
      map.list = a.features + (uint64_t)round * a.n_sel;
      grow_split_columns(a, hess, level, 0, ncols, map, batch0);
    } else {
      grow_split_columns(a, hess, level, 0, ncols, GrowIdentityMap(), batch0);
    }
    return;
  }
  grow_deep_split_chunks(a, hess, d.node_stride, level, ncols);
}

// ---- the metric ----

// one row's hq * sq into the lane's accumulators, sq < 2^64 and hq < 2^32: the three parts of grow.hpp GrowWideSum
__device__ inline void add_weighted(unsigned long long hq, unsigned long long sq, GrowWideAcc* acc) {
  const unsigned long long ha = hq * (sq >> 32), hb = hq * (sq & kGrowLow32);   // hq, a, b < 2^32: neither product overflows
  acc->p2 += ha >> 32;
  acc->p1 += (ha & kGrowLow32) + (hb >> 32);
  acc->p0 += hb & kGrowLow32;
}

// grid (blocks).  wslot: the set's W at t = 0, else nullptr
template <uint32_t METRIC>
__global__ __launch_bounds__(kBlock) void grow_sse_metric_kernel(GrowEvalArgs a, float slope, unsigned long long* slot,
                                                                 unsigned long long* wslot) {
  GrowWideAcc acc;
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    float w;
    unsigned long long hq;
    const bool sound = grow_row_weight(a.weights, row, &w, &hq);
    uint64_t sq;
    if (grow_metric_row<METRIC>(slope, a.pred[row], a.labels[row], &sq)) add_weighted(hq, sq, &acc);
    else flags |= a.label_flag;
    if (!sound) flags |= a.weight_flag;
    acc.w += hq;
  }
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, wslot);
}

// grid (blocks)
template <uint32_t METRIC>
__global__ __launch_bounds__(kBlock) void grow_walk_sse_metric_kernel(GrowEvalArgs a, float slope, uint32_t round,
                                                                      unsigned long long* slot) {
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
    uint64_t sq;
    if (grow_metric_row<METRIC>(slope, pred, a.labels[row], &sq)) add_weighted(hq, sq, &acc);
    else flags |= a.label_flag;
  }
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, nullptr);
}

// grid (blocks)
template <uint32_t METRIC>
__global__ __launch_bounds__(kBlock) void grow_deep_walk_sse_metric_kernel(GrowEvalArgs a, float slope, const EvalNode* tree,
                                                                           uint32_t node_stride, uint32_t round,
                                                                           unsigned long long* slot) {
  const uint32_t count = a.tree_nodes[round];
  GrowWideAcc acc;
  uint32_t flags = 0;
  if (count == 0 || count > node_stride) {   // (never: the split kernel writes it, and writes no record past the stride)
    flags = kGrowFlagState;
  } else {
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
      uint64_t sq;
      if (grow_metric_row<METRIC>(slope, pred, a.labels[row], &sq)) add_weighted(hq, sq, &acc);
      else flags |= a.label_flag;
    }
  }
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, nullptr);
}

bool metric_args_sound(const GrowEvalArgs& a, uint32_t metric, float slope, uint32_t blocks, uint32_t set) {
  return a.nrow != 0 && a.nrow <= kRefitMaxRows && blocks != 0 && set <= 1 && a.pred != nullptr && a.labels != nullptr &&
         a.wsums != nullptr && a.state != nullptr &&
         (metric == kGrowMetricMae || (metric == kGrowMetricPseudoHuber && grow_slope_sound(slope))) &&
         ((a.label_flag == kGrowFlagLabel && a.weight_flag == kGrowFlagWeight) ||
          (a.label_flag == kGrowFlagEvalLabel && a.weight_flag == kGrowFlagEvalWeight));
}

bool reg_sound(const GrowRegHess& h) {
  return h.min_child_weight >= 0.0 && grow_reg_sound(h.alpha) && grow_reg_sound(h.max_delta_step);
}

}  // namespace

GrowPairSplits grow_reg_splits(const GrowRegHess& hess) {
  GrowPairSplits s;
  if (!reg_sound(hess)) return s;   // (empty launches: the tree launchers refuse them)
  s.split0 = [hess](const GrowArgs& a, const uint8_t* list, uint32_t ncols, uint32_t blocks, uint32_t level, uint32_t round, void* stream) {
    const RegColumns c{list, ncols};
    hipLaunchKernelGGL((grow_split_reg_kernel<0, kGrowRootNone>), dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a, c,
                       hess, level, round);
  };
  s.split1 = [hess](const GrowArgs& a, const uint8_t* list, uint32_t ncols, int root, uint32_t level, uint32_t round, void* stream_) {
    const RegColumns c{list, ncols};
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (root == kGrowRootHess)
      hipLaunchKernelGGL((grow_split_reg_kernel<1, kGrowRootHess>), dim3(1), dim3(kBlock), 0, stream, a, c, hess, level, round);
    else if (root == kGrowRootBag)
      hipLaunchKernelGGL((grow_split_reg_kernel<1, kGrowRootBag>), dim3(1), dim3(kBlock), 0, stream, a, c, hess, level, round);
    else hipLaunchKernelGGL((grow_split_reg_kernel<1, kGrowRootNone>), dim3(1), dim3(kBlock), 0, stream, a, c, hess, level, round);
  };
  s.deep_split0 = [hess](const GrowDeepArgs& d, uint32_t level, uint32_t round, uint32_t batch0, uint32_t blocks, void* stream) {
    hipLaunchKernelGGL(grow_deep_split_reg_kernel<0>, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), d, hess, level,
                       round, batch0);
  };
  s.deep_split1 = [hess](const GrowDeepArgs& d, uint32_t level, uint32_t round, void* stream) {
    hipLaunchKernelGGL(grow_deep_split_reg_kernel<1>, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream), d, hess, level, round,
                       0u);
  };
  return s;
}

int launch_grow_sse_metric(const GrowEvalArgs& a, uint32_t metric, float slope, uint32_t blocks, uint32_t t, uint32_t set, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!metric_args_sound(a, metric, slope, blocks, set)) return hipErrorInvalidValue;
  unsigned long long* slot = a.wsums + grow_wide_index(t, set);
  unsigned long long* wslot = t == 0 ? a.wsums + set : nullptr;
  if (metric == kGrowMetricMae)
    hipLaunchKernelGGL(grow_sse_metric_kernel<kGrowMetricMae>, dim3(blocks), dim3(kBlock), 0, stream, a, slope, slot, wslot);
  else hipLaunchKernelGGL(grow_sse_metric_kernel<kGrowMetricPseudoHuber>, dim3(blocks), dim3(kBlock), 0, stream, a, slope, slot, wslot);
  return hipGetLastError();
}

int launch_grow_walk_sse_metric(const GrowEvalArgs& a, uint32_t metric, float slope, uint32_t blocks, uint32_t round, uint32_t set,
                                void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!metric_args_sound(a, metric, slope, blocks, set) || a.bins == nullptr || a.nodes == nullptr || a.tree_nodes == nullptr ||
      a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 || a.max_depth > kGrowMaxDepth)
    return hipErrorInvalidValue;
  unsigned long long* slot = a.wsums + grow_wide_index(round + 1, set);
  if (metric == kGrowMetricMae)
    hipLaunchKernelGGL(grow_walk_sse_metric_kernel<kGrowMetricMae>, dim3(blocks), dim3(kBlock), 0, stream, a, slope, round, slot);
  else hipLaunchKernelGGL(grow_walk_sse_metric_kernel<kGrowMetricPseudoHuber>, dim3(blocks), dim3(kBlock), 0, stream, a, slope, round, slot);
  return hipGetLastError();
}

int launch_grow_walk_sse_deep_metric(const GrowEvalArgs& a, const GrowDeepArgs& d, uint32_t metric, float slope, uint32_t blocks,
                                     uint32_t round, uint32_t set, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!metric_args_sound(a, metric, slope, blocks, set) || a.bins == nullptr || a.tree_nodes == nullptr || d.eval_nodes == nullptr ||
      d.node_stride == 0 || a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 ||
      a.max_depth > kGrowDeepMaxDepth)
    return hipErrorInvalidValue;
  const hipError_t e = (hipError_t)launch_grow_deep_stage(d, blocks, round, stream);
  if (e != hipSuccess) return e;
  unsigned long long* slot = a.wsums + grow_wide_index(round + 1, set);
  const EvalNode* tree = (const EvalNode*)d.eval_nodes;
  if (metric == kGrowMetricMae)
    hipLaunchKernelGGL(grow_deep_walk_sse_metric_kernel<kGrowMetricMae>, dim3(blocks), dim3(kBlock), 0, stream, a, slope, tree,
                       d.node_stride, round, slot);
  else
    hipLaunchKernelGGL(grow_deep_walk_sse_metric_kernel<kGrowMetricPseudoHuber>, dim3(blocks), dim3(kBlock), 0, stream, a, slope, tree,
                       d.node_stride, round, slot);
  return hipGetLastError();
}

}  // namespace ohx
