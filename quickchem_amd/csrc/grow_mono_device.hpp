// What the kernel files of constrained boosting share (grow_mono.hip, grow_colsample.hip), each written once: how phase 1
// decides a node and writes a split where the call's policy is GrowMonoArgs (grow.hpp; design in
// docs/28_monotone_constraints.md).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_device.hpp"

namespace ohx {

// Phase 1 decides a node and writes a split through grow_decide_node and grow_write_split, which take the call's policy.
// For GrowMonoArgs these two overloads are the more specialised, so grow_split_nodes and grow_deep_split_chunks, which
// name neither policy, find them at their instantiation in the kernel files: each builds the policy of its node and hands
// over to the shared function.  The feature's constraint plays no part in a leaf solve or in which nodes are looked at, so
// a node is decided with c = 0; a split is written with the constraint of the feature it splits on.
template <bool BAG>
__device__ inline GrowDecision grow_decide_node(const GrowArgs& a, const GrowMonoArgs& m, GrowNode* nodes, uint32_t level,
                                                uint32_t node, uint32_t slot, uint32_t ncols) {
  GrowMonoHess h = m.at(node, 0);
  h.c = 0;
  return grow_decide_node<BAG>(a, h, nodes, level, node, slot, ncols);
}
// The children's weights lie in their own intervals (wL <= mid <= wR or the reverse, both within the parent's), so the
// leaf records written under the parent's interval are those under their own.  The caller has checked left + 1 against
// the node stride, which is the array's.
__device__ inline void grow_write_split(const GrowArgs& a, const GrowMonoArgs& m, GrowNode* nodes, uint32_t node,
                                        const GrowDecision& d, uint32_t left) {
  const GrowMonoHess h = m.at(node, d.best.key >> 9);
  double iv[4];
  h.children(d.best.GL, d.best.HL, d.Gp - d.best.GL, d.Hp - d.best.HL, (double)a.lambda, iv);
  double* at = m.bounds + 2 * (uint64_t)left;
  at[0] = iv[0];
  at[1] = iv[1];
  at[2] = iv[2];
  at[3] = iv[3];
  grow_write_split(a, h, nodes, node, d, left);
}

}  // namespace ohx
#endif  // __HIPCC__
