// gfx950 kernels of boosting under interaction constraints (grow.hpp GrowInteractArgs; design in
// docs/35_interaction_constraints.md).  A call runs them only where "ohx_interaction_constraints" is active: with the
// default, or a group that holds every feature, nothing of this file is touched, its code object included.
//
//   grow_split_interact_kernel<P, 0, ..>     levels 0 - 7: grow_device.hpp's phase 0 over the tree's list under the
//                                            policy P of the call.  A wave whose feature is not in its node's allowed
//                                            set leaves an invalid candidate and reads no histogram; at level 0 the wave
//                                            of column 0 still leaves the root's sums.
//   grow_split_interact_kernel<P, 1, ROOT>   its phase 1: P's own decision and records, and the children's sets beside
//                                            their leaf records.  ROOT is grow_split_pairs_kernel's.
//   grow_deep_split_interact_kernel<P, 0>    levels 8 - 17, once per batch: the same phase 0 over the batch's histograms.
//   grow_deep_split_interact_kernel<P, 1>    once per level, one block: grow_deep_device.hpp's chunked walk.
// P is GrowFixedHess, GrowRegHess or GrowMonoArgs: the gain, the order of the candidates, the leaf solve and the records
// are theirs, through grow_split_columns, grow_split_nodes and grow_deep_split_chunks.
// The sets are four words a node id - the features on the node's path, then the features it may split on - in one array
// of the tree at hand, which both paths index alike: level 8 reads what level 7 wrote.  Node 0's sets are ({}, every
// feature) and are never read, and every other node's are written when its parent splits, before any kernel that reads
// them is enqueued: nothing is reset between trees.  The pair kernel, both pair histogram kernels, and the bin, partition,
// leaf, widen, stage, walk and metric kernels are the other files' own.  Plain stores, integer adds and bit operations:
// no float atomics, no compare-and-swap loops, and no atomic beyond the error word's or.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_deep_device.hpp"
#include "grow_device.hpp"
#include "grow_interact_device.hpp"
#include "grow_mono_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;

// the histogram columns of the tree at hand: column k is feature list[k]
struct InteractColumns {
  const uint8_t* list;
  uint32_t ncols;
};

// the policy of one (node, feature): the call's own, or under monotone constraints the node's interval and the feature's
// constraint
__device__ inline const GrowFixedHess& policy_at(const GrowFixedHess& h, uint32_t, uint32_t) { return h; }
__device__ inline const GrowRegHess& policy_at(const GrowRegHess& h, uint32_t, uint32_t) { return h; }
__device__ inline GrowMonoHess policy_at(const GrowMonoArgs& m, uint32_t node, uint32_t f) { return m.at(node, f); }

// Phase 0 of either path: the wave's slot and column as grow_split_columns works them out, then grow_split_columns itself
// where the column's feature is in the node's allowed set.  The node is the same in every lane of the wave: 16 bytes a
// wave, and none for the root.
template <class Policy, class Map>
__device__ inline void interact_columns(const GrowArgs& a, const GrowInteractArgs<Policy>& x, uint32_t level, uint32_t round,
                                        uint32_t ncols, Map map, uint32_t slot0) {
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t w = blockIdx.x * (kGrowBlock / kWave) + threadIdx.x / kWave;
  const uint32_t slot = slot0 + w / ncols, k = w % ncols;
  if (slot >= end - begin) return;
  const uint32_t node = begin + slot;
  const uint32_t f = map(k);
  uint64_t allowed[2];
  grow_interact_node_allowed(x, node, a.num_feature, allowed);
  const bool member = grow_interact_has(allowed, f);
  // (the root's sums are column 0's to leave, whether or not the root may split on it)
  if (member || (level == 0 && k == 0)) grow_split_columns(a, policy_at(x.inner, node, f), level, round, ncols, map, slot0);
  if (!member && lane == 0) a.best[(uint64_t)slot * ncols + k] = GrowCand();
}

// PHASE 0: grid (blocks of four waves over slots x columns).  PHASE 1: one block.
template <class Policy, int PHASE, int ROOT>
__global__ __launch_bounds__(kBlock) void grow_split_interact_kernel(GrowArgs a, InteractColumns c, GrowInteractArgs<Policy> x,
                                                                     uint32_t level, uint32_t round) {
  if (PHASE == 0) {
    GrowListMap map;
    map.list = c.list;
    interact_columns(a, x, level, round, c.ncols, map, 0);
  } else {
    grow_split_nodes<ROOT == kGrowRootBag>(a, x, level, round, c.ncols);
    // the root's sums are phase 0's, written before this kernel started
    if (ROOT == kGrowRootHess && level == 0 && threadIdx.x == 0 && a.nodes[(uint64_t)round * kGrowMaxNodes].H == 0)
      atomicOr(&a.state->error, kGrowFlagHess);
  }
}

// PHASE 0: grid (blocks of four waves over the batch's slots x columns).  PHASE 1: one block.  With d.g.features the
// columns are the tree's list, else every feature.
template <class Policy, int PHASE>
__global__ __launch_bounds__(kBlock) void grow_deep_split_interact_kernel(GrowDeepArgs d, GrowInteractArgs<Policy> x, uint32_t level,
                                                                          uint32_t round, uint32_t batch0) {
  const GrowArgs a = grow_deep_tree_args(d, round);
  const bool listed = a.features != nullptr;
  const uint32_t ncols = listed ? a.n_sel : a.num_feature;
  if (PHASE == 0) {
    if (listed) {
      GrowListMap map;
      map.list = a.features + (uint64_t)round * a.n_sel;
      interact_columns(a, x, level, 0, ncols, map, batch0);
    } else {
      interact_columns(a, x, level, 0, ncols, GrowIdentityMap(), batch0);
    }
    return;
  }
  grow_deep_split_chunks(a, x, d.node_stride, level, ncols);
}

bool policy_sound(const GrowFixedHess& h) { return h.min_child_weight >= 0.0; }
bool policy_sound(const GrowRegHess& h) {
  return h.min_child_weight >= 0.0 && grow_reg_sound(h.alpha) && grow_reg_sound(h.max_delta_step);
}
bool policy_sound(const GrowMonoArgs& m) { return policy_sound(m.reg) && m.bounds != nullptr && m.constraints != nullptr; }

template <class Policy>
GrowPairSplits interact_splits(const GrowInteractArgs<Policy>& x) {
  GrowPairSplits s;
  // (empty launches: the tree launchers refuse them)
  if (x.groups == nullptr || x.sets == nullptr || x.ngroups < 1 || x.ngroups > kGrowMaxGroups || !policy_sound(x.inner)) return s;
  s.split0 = [x](const GrowArgs& a, const uint8_t* list, uint32_t ncols, uint32_t blocks, uint32_t level, uint32_t round, void* stream) {
    const InteractColumns c{list, ncols};
    hipLaunchKernelGGL((grow_split_interact_kernel<Policy, 0, kGrowRootNone>), dim3(blocks), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a, c, x, level, round);
  };
  s.split1 = [x](const GrowArgs& a, const uint8_t* list, uint32_t ncols, int root, uint32_t level, uint32_t round, void* stream_) {
    const InteractColumns c{list, ncols};
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (root == kGrowRootHess)
      hipLaunchKernelGGL((grow_split_interact_kernel<Policy, 1, kGrowRootHess>), dim3(1), dim3(kBlock), 0, stream, a, c, x, level, round);
    else if (root == kGrowRootBag)
      hipLaunchKernelGGL((grow_split_interact_kernel<Policy, 1, kGrowRootBag>), dim3(1), dim3(kBlock), 0, stream, a, c, x, level, round);
    else
      hipLaunchKernelGGL((grow_split_interact_kernel<Policy, 1, kGrowRootNone>), dim3(1), dim3(kBlock), 0, stream, a, c, x, level, round);
  };
  s.deep_split0 = [x](const GrowDeepArgs& d, uint32_t level, uint32_t round, uint32_t batch0, uint32_t blocks, void* stream) {
    hipLaunchKernelGGL((grow_deep_split_interact_kernel<Policy, 0>), dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), d,
                       x, level, round, batch0);
  };
  s.deep_split1 = [x](const GrowDeepArgs& d, uint32_t level, uint32_t round, void* stream) {
    hipLaunchKernelGGL((grow_deep_split_interact_kernel<Policy, 1>), dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream), d, x,
                       level, round, 0u);
  };
  return s;
}

}  // namespace

GrowPairSplits grow_interact_splits(const GrowInteractArgs<GrowFixedHess>& x) { return interact_splits(x); }
GrowPairSplits grow_interact_splits(const GrowInteractArgs<GrowRegHess>& x) { return interact_splits(x); }
GrowPairSplits grow_interact_splits(const GrowInteractArgs<GrowMonoArgs>& x) { return interact_splits(x); }

}  // namespace ohx
