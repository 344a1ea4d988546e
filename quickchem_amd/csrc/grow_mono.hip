// gfx950 kernels of boosting under monotone constraints (grow.hpp GrowMonoHess, GrowMonoArgs; design in
// docs/28_monotone_constraints.md).  A call runs them only where "ohx_monotone_constraints" holds an entry that is not 0:
// with the default, or a list of zeros, nothing of this file is touched, its code object included.
//
//   grow_split_mono_kernel<0, ..>       levels 0 - 7: grow_device.hpp's phase 0 over the pair path's feature list, with the
//                                       policy of the wave's (node, feature): the node's interval and the feature's
//                                       constraint.  The scan admits a candidate by both children's weights too.
//   grow_split_mono_kernel<1, ROOT>     its phase 1: the leaf solve under the node's interval, and the children's
//                                       intervals beside their leaf records.  ROOT is grow_split_pairs_kernel's.
//   grow_deep_split_mono_kernel<0>      levels 8 - 17, once per batch: the same phase 0 over the batch's histograms.
//   grow_deep_split_mono_kernel<1>      once per level, one block: grow_deep_device.hpp's chunked walk.
// The intervals are two doubles a node id in one array of the tree at hand, which both paths index alike: level 8 reads
// what level 7 wrote.  Node 0's interval is (-inf, +inf) and is never read, and every other node's is written when its
// parent splits, before any kernel that reads it is enqueued: nothing is reset between trees.  The pair kernel, both pair
// histogram kernels, and the bin, partition, leaf, widen, stage, walk and metric kernels are the other files' own.
// Plain stores and integer adds: no float atomics, no compare-and-swap loops.
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

// the histogram columns of the tree at hand: column k is feature list[k]
struct MonoColumns {
  const uint8_t* list;
  uint32_t ncols;
};

// Phase 0 of either path: grow_split_columns with the policy of the wave's own (node, feature), worked out as
// grow_split_columns works out its slot and column.  A wave without a slot builds no policy and reads no interval.
template <class Map>
__device__ inline void mono_split_columns(const GrowArgs& a, const GrowMonoArgs& m, uint32_t level, uint32_t round, uint32_t ncols,
                                          Map map, uint32_t slot0) {
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t w = blockIdx.x * (kGrowBlock / kWave) + threadIdx.x / kWave;
  const uint32_t slot = slot0 + w / ncols;
  if (slot >= end - begin) return;
  grow_split_columns(a, m.at(begin + slot, map(w % ncols)), level, round, ncols, map, slot0);
}

// PHASE 0: grid (blocks of four waves over slots x columns).  PHASE 1: one block.
template <int PHASE, int ROOT>
__global__ __launch_bounds__(kBlock) void grow_split_mono_kernel(GrowArgs a, MonoColumns c, GrowMonoArgs m, uint32_t level,
                                                                 uint32_t round) {
  if (PHASE == 0) {
    GrowListMap map;
    map.list = c.list;
    mono_split_columns(a, m, level, round, c.ncols, map, 0);
  } else {
    grow_split_nodes<ROOT == kGrowRootBag>(a, m, level, round, c.ncols);
    // the root's sums are phase 0's, written before this kernel started
    if (ROOT == kGrowRootHess && level == 0 && threadIdx.x == 0 && a.nodes[(uint64_t)round * kGrowMaxNodes].H == 0)
      atomicOr(&a.state->error, kGrowFlagHess);
  }
}

// PHASE 0: grid (blocks of four waves over the batch's slots x columns).  PHASE 1: one block.  With d.g.features the
// columns are the tree's list, else every feature.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void grow_deep_split_mono_kernel(GrowDeepArgs d, GrowMonoArgs m, uint32_t level, uint32_t round,
                                                                      uint32_t batch0) {
  const GrowArgs a = grow_deep_tree_args(d, round);
  const bool listed = a.features != nullptr;
  const uint32_t ncols = listed ? a.n_sel : a.num_feature;
  if (PHASE == 0) {
    if (listed) {
      GrowListMap map;
      map.list = a.features + (uint64_t)round * a.n_sel;
      mono_split_columns(a, m, level, 0, ncols, map, batch0);
    } else {
      mono_split_columns(a, m, level, 0, ncols, GrowIdentityMap(), batch0);
    }
    return;
  }
  grow_deep_split_chunks(a, m, d.node_stride, level, ncols);
}

bool mono_sound(const GrowMonoArgs& m) {
  return m.reg.min_child_weight >= 0.0 && grow_reg_sound(m.reg.alpha) && grow_reg_sound(m.reg.max_delta_step) && m.bounds != nullptr &&
         m.constraints != nullptr;
}

}  // namespace

GrowPairSplits grow_mono_splits(const GrowMonoArgs& m) {
  GrowPairSplits s;
  if (!mono_sound(m)) return s;   // (empty launches: the tree launchers refuse them)
  s.split0 = [m](const GrowArgs& a, const uint8_t* list, uint32_t ncols, uint32_t blocks, uint32_t level, uint32_t round, void* stream) {
    const MonoColumns c{list, ncols};
    hipLaunchKernelGGL((grow_split_mono_kernel<0, kGrowRootNone>), dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a, c,
                       m, level, round);
  };
  s.split1 = [m](const GrowArgs& a, const uint8_t* list, uint32_t ncols, int root, uint32_t level, uint32_t round, void* stream_) {
    const MonoColumns c{list, ncols};
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (root == kGrowRootHess)
      hipLaunchKernelGGL((grow_split_mono_kernel<1, kGrowRootHess>), dim3(1), dim3(kBlock), 0, stream, a, c, m, level, round);
    else if (root == kGrowRootBag)
      hipLaunchKernelGGL((grow_split_mono_kernel<1, kGrowRootBag>), dim3(1), dim3(kBlock), 0, stream, a, c, m, level, round);
    else hipLaunchKernelGGL((grow_split_mono_kernel<1, kGrowRootNone>), dim3(1), dim3(kBlock), 0, stream, a, c, m, level, round);
  };
  s.deep_split0 = [m](const GrowDeepArgs& d, uint32_t level, uint32_t round, uint32_t batch0, uint32_t blocks, void* stream) {
    hipLaunchKernelGGL(grow_deep_split_mono_kernel<0>, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), d, m, level,
                       round, batch0);
  };
  s.deep_split1 = [m](const GrowDeepArgs& d, uint32_t level, uint32_t round, void* stream) {
    hipLaunchKernelGGL(grow_deep_split_mono_kernel<1>, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream), d, m, level, round,
                       0u);
  };
  return s;
}

}  // namespace ohx
