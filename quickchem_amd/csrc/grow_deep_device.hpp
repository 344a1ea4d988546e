// What the kernel files of the deep levels share (grow_deep.hip, grow_reg.hip), each written once: the tree at hand as
// round 0 of its own table, and split phase 1 of a deep level over a hessian policy (grow.hpp).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_device.hpp"
#include "walk_device.hpp"

namespace ohx {

constexpr int kGrowDeepWaves = (int)kGrowBlock / kWave;

// The tree at hand as round 0 of its own table: what the shared split phases and the weighted levels index by round.
__host__ __device__ inline GrowArgs grow_deep_tree_args(const GrowDeepArgs& a, uint32_t round) {
  GrowArgs t = a.g;
  t.nodes = a.g.nodes + (uint64_t)round * a.node_stride;
  t.tree_nodes = a.g.tree_nodes + round;
  return t;
}

// Split phase 1 of a deep level, written once for every kind and policy: one block of kGrowBlock lanes walks the level's
// slots in chunks of its width with a running total (grow.hpp grow_chunked_children) and decides every node over `ncols`
// columns of `best`.
template <class Hess>
__device__ inline void grow_deep_split_chunks(const GrowArgs& a, const Hess& hess, uint32_t node_stride, uint32_t level,
                                              uint32_t ncols) {
  constexpr int kBlock = (int)kGrowBlock;
  constexpr int kWaves = kGrowDeepWaves;
  __shared__ uint32_t wave_splits[kWaves];
  const uint32_t begin = a.state->begin, end = a.state->end, next = a.state->next;
  const uint32_t count = end - begin;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint32_t running = 0;   // the splits of the chunks before this one: the same in every lane
  bool full = false;      // a child id past the round's records (never: grow_deep_node_stride)
  for (uint32_t c0 = 0; c0 < count; c0 += kBlock) {
    const uint32_t s = c0 + threadIdx.x;
    const uint32_t node = begin + s;
    GrowDecision dec;
    if (s < count) dec = grow_decide_node<false>(a, hess, a.nodes, level, node, s, ncols);
    const bool split = s < count && dec.split;
    // the exclusive scan of the chunk's flags: the lanes below in the wave, and the waves below in the block
    const unsigned long long votes = __ballot(split);
    if (lane == 0) wave_splits[wave] = (uint32_t)__popcll(votes);
    __syncthreads();
    uint32_t scan = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull)), chunk = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) scan += wave_splits[w];
      chunk += wave_splits[w];
    }
    __syncthreads();   // wave_splits is written again in the next chunk
    if (split) {
      const uint32_t left = grow_child_id(next, running + scan);
      if (left + 1u < node_stride) grow_write_split(a, hess, a.nodes, node, dec, left);
      else full = true;
    }
    running += chunk;
  }
  if (full) atomicOr(&a.state->error, kGrowFlagState);
  uint32_t total = next + 2u * running;
  if (total > node_stride) total = next;   // (never; the flag is raised above) nothing is open: the tree ends
  __syncthreads();
  if (threadIdx.x == 0) {
    a.state->begin = next;
    a.state->end = total;
    a.state->next = total;
    a.tree_nodes[0] = total;
  }
}

}  // namespace ohx
#endif  // __HIPCC__
