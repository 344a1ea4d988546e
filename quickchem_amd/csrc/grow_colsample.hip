// gfx950 kernels of boosting with column sampling by level and by node (grow.hpp GrowColsampleArgs; design in
// docs/29_colsample_level_node.md).  A call runs them only where "ohx_colsample_bylevel" or "ohx_colsample_bynode" takes
// a feature away from a level or a node: with n_lvl == n_sel and n_node == n_lvl, the defaults included, nothing of this
// file is touched, its code object included.
//
//   grow_split_colsample_kernel<P, 0, ..>     levels 0 - 7: grow_device.hpp's phase 0 over the level's list under the
//                                             policy P of the call.  A wave whose column is not one of its node's
//                                             features leaves an invalid candidate and reads no histogram; at level 0
//                                             the wave of column 0 still leaves the root's sums.
//   grow_split_colsample_kernel<P, 1, ROOT>   its phase 1 over the n_lvl columns of a slot.  ROOT is
//                                             grow_split_pairs_kernel's.
//   grow_deep_split_colsample_kernel<P, 0>    levels 8 - 17, once per batch: the same phase 0 over the batch's histograms.
//   grow_deep_split_colsample_kernel<P, 1>    once per level, one block: grow_deep_device.hpp's chunked walk.
// P is GrowFixedHess, GrowRegHess or GrowMonoArgs: the gain, the order of the candidates, the leaf solve and the records
// are theirs, through grow_split_columns, grow_split_nodes and grow_deep_split_chunks.
// Whether a column is one of a node's features is a rank, computed by the wave that owns the (node, column) and stored
// nowhere: the lanes make the keys mix(K_node + f_j) of the level's n_lvl <= 128 features, at most two a lane, and those
// below the wave's own (key, f) are counted by ballot and popcount.  The column is in where they are fewer than n_node.
// The pair kernel, both pair histogram kernels - launched over the level's list by the host - and the bin, partition, leaf,
// widen, stage, walk and metric kernels are the other files' own.  Plain stores and integer adds: no float atomics, no
// compare-and-swap loops, and no atomic beyond the error word's or.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_deep_device.hpp"
#include "grow_device.hpp"
#include "grow_mono_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;
static_assert(kGrowMaxFeatures <= 2 * kWave, "a lane makes at most two keys of a level's list");

// the policy of one (node, feature): the call's own, or under monotone constraints the node's interval and the feature's
// constraint
__device__ inline const GrowFixedHess& policy_at(const GrowFixedHess& h, uint32_t, uint32_t) { return h; }
__device__ inline const GrowRegHess& policy_at(const GrowRegHess& h, uint32_t, uint32_t) { return h; }
__device__ inline GrowMonoHess policy_at(const GrowMonoArgs& m, uint32_t node, uint32_t f) { return m.at(node, f); }

// Whether feature f of the level's list is one of node `node`'s features: grow.hpp grow_node_has_feature with the list
// spread over the lanes.  The same in every lane of the wave; every lane of the wave must call it.
__device__ inline bool colsample_member(const GrowColsampleArgs& c, const uint8_t* list, uint64_t col_key, uint32_t node, uint32_t f,
                                        int lane) {
  if (c.n_node >= c.n_lvl) return true;
  const uint64_t key = grow_node_key(col_key, node);
  const uint64_t mine = grow_mix(key + f);
  uint32_t below = 0;
#pragma unroll
  for (uint32_t j = 0; j < 2; ++j) {
    const uint32_t k = (uint32_t)lane + j * kWave;
    bool lower = false;
    if (k < c.n_lvl) {
      const uint32_t fk = list[k];
      lower = grow_draw_below(grow_mix(key + fk), fk, mine, f);
    }
    below += (uint32_t)__popcll(__ballot(lower));
  }
  return below < c.n_node;
}

// Phase 0 of either path: the wave's slot and column as grow_split_columns works them out, then grow_split_columns itself
// where the column is the node's.  `round` indexes the node records, `tree` the lists and the draw: the call's round.
template <class Policy>
__device__ inline void colsample_columns(const GrowArgs& a, const Policy& pol, const GrowColsampleArgs& c, uint32_t level,
                                         uint32_t round, uint32_t tree, uint32_t slot0) {
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t w = blockIdx.x * (kGrowBlock / kWave) + threadIdx.x / kWave;
  const uint32_t ncols = c.n_lvl;
  const uint32_t slot = slot0 + w / ncols, k = w % ncols;
  if (slot >= end - begin || level >= c.depth) return;
  const uint32_t node = begin + slot;
  GrowListMap map;
  map.list = c.list(tree, level);
  const uint32_t f = map(k);
  const bool member = colsample_member(c, map.list, c.col_key(tree), node, f, lane);
  // (the root's sums are column 0's to leave, whether or not the root may split on it)
  if (member || (level == 0 && k == 0)) grow_split_columns(a, policy_at(pol, node, f), level, round, ncols, map, slot0);
  if (!member && lane == 0) a.best[(uint64_t)slot * ncols + k] = GrowCand();
}

// PHASE 0: grid (blocks of four waves over slots x n_lvl).  PHASE 1: one block.
template <class Policy, int PHASE, int ROOT>
__global__ __launch_bounds__(kBlock) void grow_split_colsample_kernel(GrowArgs a, GrowColsampleArgs c, Policy pol, uint32_t level,
                                                                      uint32_t round, uint32_t tree) {
  if (PHASE == 0) {
    colsample_columns(a, pol, c, level, round, tree, 0);
  } else {
    grow_split_nodes<ROOT == kGrowRootBag>(a, pol, level, round, c.n_lvl);
    // the root's sums are phase 0's, written before this kernel started
    if (ROOT == kGrowRootHess && level == 0 && threadIdx.x == 0 && a.nodes[(uint64_t)round * kGrowMaxNodes].H == 0)
      atomicOr(&a.state->error, kGrowFlagHess);
  }
}

// PHASE 0: grid (blocks of four waves over the batch's slots x n_lvl).  PHASE 1: one block.
template <class Policy, int PHASE>
__global__ __launch_bounds__(kBlock) void grow_deep_split_colsample_kernel(GrowDeepArgs d, GrowColsampleArgs c, Policy pol,
                                                                           uint32_t level, uint32_t round, uint32_t batch0) {
  const GrowArgs a = grow_deep_tree_args(d, round);
  if (PHASE == 0) colsample_columns(a, pol, c, level, 0, round, batch0);
  else grow_deep_split_chunks(a, pol, d.node_stride, level, c.n_lvl);
}

bool colsample_sound(const GrowColsampleArgs& c) {
  return c.lists != nullptr && c.depth >= 1 && c.depth <= (uint32_t)kGrowDeepMaxDepth && c.n_node >= 1 && c.n_node <= c.n_lvl &&
         c.n_lvl <= kGrowMaxFeatures;
}
bool policy_sound(const GrowFixedHess& h) { return h.min_child_weight >= 0.0; }
bool policy_sound(const GrowRegHess& h) {
  return h.min_child_weight >= 0.0 && grow_reg_sound(h.alpha) && grow_reg_sound(h.max_delta_step);
}
bool policy_sound(const GrowMonoArgs& m) { return policy_sound(m.reg) && m.bounds != nullptr && m.constraints != nullptr; }

template <class Policy>
GrowPairSplits colsample_splits(const GrowColsampleArgs& c, const Policy& pol) {
  GrowPairSplits s;
  if (!colsample_sound(c) || !policy_sound(pol)) return s;   // (empty launches: the tree launchers refuse them)
  s.levels = c;
  s.level_split0 = [c, pol](const GrowArgs& a, uint32_t tree, uint32_t blocks, uint32_t level, uint32_t round, void* stream) {
    hipLaunchKernelGGL((grow_split_colsample_kernel<Policy, 0, kGrowRootNone>), dim3(blocks), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a, c, pol, level, round, tree);
  };
  s.level_split1 = [c, pol](const GrowArgs& a, uint32_t tree, int root, uint32_t level, uint32_t round, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (root == kGrowRootHess)
      hipLaunchKernelGGL((grow_split_colsample_kernel<Policy, 1, kGrowRootHess>), dim3(1), dim3(kBlock), 0, stream, a, c, pol, level,
                         round, tree);
    else if (root == kGrowRootBag)
      hipLaunchKernelGGL((grow_split_colsample_kernel<Policy, 1, kGrowRootBag>), dim3(1), dim3(kBlock), 0, stream, a, c, pol, level,
                         round, tree);
    else
      hipLaunchKernelGGL((grow_split_colsample_kernel<Policy, 1, kGrowRootNone>), dim3(1), dim3(kBlock), 0, stream, a, c, pol, level,
                         round, tree);
  };
  s.deep_split0 = [c, pol](const GrowDeepArgs& d, uint32_t level, uint32_t round, uint32_t batch0, uint32_t blocks, void* stream) {
    hipLaunchKernelGGL((grow_deep_split_colsample_kernel<Policy, 0>), dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       d, c, pol, level, round, batch0);
  };
  s.deep_split1 = [c, pol](const GrowDeepArgs& d, uint32_t level, uint32_t round, void* stream) {
    hipLaunchKernelGGL((grow_deep_split_colsample_kernel<Policy, 1>), dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream), d, c,
                       pol, level, round, 0u);
  };
  return s;
}

}  // namespace

GrowPairSplits grow_colsample_splits(const GrowColsampleArgs& c, const GrowFixedHess& hess) { return colsample_splits(c, hess); }
GrowPairSplits grow_colsample_splits(const GrowColsampleArgs& c, const GrowRegHess& hess) { return colsample_splits(c, hess); }
GrowPairSplits grow_colsample_splits(const GrowColsampleArgs& c, const GrowMonoArgs& m) { return colsample_splits(c, m); }

}  // namespace ohx
