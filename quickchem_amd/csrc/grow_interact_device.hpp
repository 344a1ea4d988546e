// How phase 1 decides a node and writes a split where the call's policy is GrowInteractArgs (grow.hpp; design in
// docs/35_interaction_constraints.md), for grow_interact.hip.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_device.hpp"
#include "grow_mono_device.hpp"

namespace ohx {

// The allowed set of a node as a split kernel reads it: the root's is every feature, without a read.
template <class Policy>
__device__ inline void grow_interact_node_allowed(const GrowInteractArgs<Policy>& x, uint32_t node, uint32_t F, uint64_t out[2]) {
  if (node == 0) {
    grow_interact_all(F, out);
  } else {
    out[0] = x.sets[4 * (uint64_t)node + 2];
    out[1] = x.sets[4 * (uint64_t)node + 3];
  }
}

// As grow_mono_device.hpp's: for GrowInteractArgs these two overloads are the more specialised, so grow_split_nodes and
// grow_deep_split_chunks find them at their instantiation in the kernel file.  The constraints play no part in a leaf
// solve or in which nodes are looked at - phase 0 has left the columns outside the node's set invalid - so a node is
// decided by the inner policy as it is.
template <bool BAG, class Policy>
__device__ inline GrowDecision grow_decide_node(const GrowArgs& a, const GrowInteractArgs<Policy>& x, GrowNode* nodes, uint32_t level,
                                                uint32_t node, uint32_t slot, uint32_t ncols) {
  return grow_decide_node<BAG>(a, x.inner, nodes, level, node, slot, ncols);
}
// The inner policy's records (under monotone constraints the children's intervals too), then both children's sets beside
// their leaf records: P(c) = P(p) with the split's feature, A(c) by grow_interact_allowed.  Both children get the same
// eight words.  The caller has checked left + 1 against the node stride, which is the array's.
template <class Policy>
__device__ inline void grow_write_split(const GrowArgs& a, const GrowInteractArgs<Policy>& x, GrowNode* nodes, uint32_t node,
                                        const GrowDecision& d, uint32_t left) {
  grow_write_split(a, x.inner, nodes, node, d, left);
  const uint32_t f = d.best.key >> 9;
  uint64_t P[2] = {0, 0}, A[2];
  if (node != 0) {
    P[0] = x.sets[4 * (uint64_t)node];
    P[1] = x.sets[4 * (uint64_t)node + 1];
  }
  const uint64_t bit = 1ull << (f & 63u);   // (f < 128: no dynamic index into P)
  if (f < 64) P[0] |= bit;
  else P[1] |= bit;
  grow_interact_allowed(P, x.groups, x.ngroups, a.num_feature, A);
  uint64_t* at = x.sets + 4 * (uint64_t)left;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    at[4 * c + 0] = P[0];
    at[4 * c + 1] = P[1];
    at[4 * c + 2] = A[0];
    at[4 * c + 3] = A[1];
  }
}

}  // namespace ohx
#endif  // __HIPCC__
