// The leaves of quantile boosting (include/ohxgb.h "ohx_objective" = quantile; design in docs/32_quantile_objective.md).
// The pinball loss has a constant hessian, so a Newton leaf counts votes; the leaf of a quantile tree is the lower weighted
// alpha-quantile of the residuals label - pred of the rows that end on it, with no interpolation: with k = cuts_key(bits(r))
// (cuts.hpp: the order of the floats as unsigned integers, -0.0f as +0.0f), W = sum hq and C(k) = sum of hq over keys <= k,
// the smallest key k* with alpha_q * W <= 2^24 * C(k*), in exact integers.  The device finds it by a radix select, 8 key
// bits a pass from the top: a pass adds hq into the 256 bins of the next digit for the rows whose key matches the leaf's
// prefix so far, and a pick takes the first digit at which the rule holds.
//
// What host and device share is here: the rule, the pick of one digit from a leaf's 256 bins, and the leaf value.  The
// host's whole select (grow_host.cpp) is written over the same functions.
#pragma once
#include <cstdint>

#include "cuts.hpp"
#include "grow.hpp"

namespace ohx {

constexpr uint32_t kGrowQuantilePasses = 4;        // of 8 key bits each, most significant first
constexpr uint32_t kGrowQuantileDigits = 256;      // bins of a pass
constexpr uint32_t kGrowQuantileMaxLeaves = 256;   // a tree of depth 8
constexpr uint32_t kGrowQuantileGroup = 64;        // leaves whose bins a block of the pass kernel holds in LDS: 128 KiB
constexpr uint32_t kGrowQuantileNoSlot = 0xFFFFu;  // a node that is no leaf

// alpha_q * W <= 2^24 * C as the exact integers: alpha_q <= 2^24 and W, C < 2^63, so both sides lie below 2^88
OHX_GROW_HD inline bool grow_quantile_reached(uint32_t alpha_q, uint64_t W, uint64_t C) {
  return (unsigned __int128)alpha_q * (unsigned __int128)W <= ((unsigned __int128)C << 24);
}

// the key of a row's residual and its digit in pass `pass`
OHX_GROW_HD inline uint32_t grow_quantile_key(float pred, float label) { return cuts_key(cuts_float_bits(label - pred)); }
OHX_GROW_HD inline uint32_t grow_quantile_digit(uint32_t key, uint32_t pass) { return (key >> (24u - 8u * pass)) & 255u; }
// whether a key carries the prefix a leaf has after `pass` picks (the top 8 * pass bits)
OHX_GROW_HD inline bool grow_quantile_matches(uint32_t key, uint32_t prefix, uint32_t pass) {
  return pass == 0 || (key >> (32u - 8u * pass)) == prefix;
}

// One leaf between passes: the digits picked so far, the weight of the keys below that prefix, and the leaf's weight
// (known after the first pass: the sum of its 256 bins)
struct GrowQuantileLeaf {
  uint32_t prefix = 0;
  uint64_t below = 0;
  uint64_t W = 0;
};

// The pick of one pass over the leaf's bins of that pass, serially: the first digit d with
// alpha_q * W <= 2^24 * (below + bins[0] + .. + bins[d]).  A leaf without weight picks nothing (false).  One exists
// otherwise: the bins of a pass sum to the weight of the digit picked before, at which the rule held.
OHX_GROW_HD inline bool grow_quantile_pick(const uint64_t* bins, uint32_t pass, uint32_t alpha_q, GrowQuantileLeaf* leaf) {
  if (pass == 0) {
    uint64_t W = 0;
    for (uint32_t d = 0; d < kGrowQuantileDigits; ++d) W += bins[d];
    leaf->W = W;
    leaf->below = 0;
    leaf->prefix = 0;
  }
  if (leaf->W == 0) return false;
  uint64_t cum = leaf->below;
  for (uint32_t d = 0; d < kGrowQuantileDigits; ++d) {
    if (grow_quantile_reached(alpha_q, leaf->W, cum + bins[d])) {
      leaf->below = cum;
      leaf->prefix = (leaf->prefix << 8) | d;
      return true;
    }
    cum += bins[d];
  }
  return false;   // (never, from bins that are the leaf's)
}

// q_p and the leaf value from the key picked: one float32 multiply, the one refit_solve_leaf ends with
OHX_GROW_HD inline float grow_quantile_value(uint32_t key, float eta) {
  return __builtin_bit_cast(float, cuts_unkey(key)) * eta;
}

// The launch shape of grow_quantile_pass_kernel for a tree of `max_depth` levels over `nrow` rows, where the streaming
// kernels of the call take `row_blocks` blocks (GrowPlan::row_blocks: kGrowRowBlocksPerCu a CU at most).  A block holds
// the bins of `group` leaves and a CU's LDS, so the grid is about a block a CU over all of its `groups`; a block takes
// kGrowHistBlock rows a trip.
struct GrowQuantilePlan {
  uint32_t group = 0;    // leaves a block holds
  uint32_t groups = 0;   // gridDim.y: group * groups >= 2^max_depth
  uint32_t blocks = 0;   // gridDim.x, at least 1
};
inline GrowQuantilePlan plan_grow_quantile(uint64_t nrow, int max_depth, uint32_t row_blocks) {
  GrowQuantilePlan p;
  const uint32_t leaves = 1u << max_depth;
  p.group = leaves < kGrowQuantileGroup ? leaves : kGrowQuantileGroup;
  p.groups = (leaves + p.group - 1) / p.group;
  const uint64_t want = (nrow + kGrowHistBlock - 1) / kGrowHistBlock, cap = row_blocks / (kGrowRowBlocksPerCu * p.groups);
  const uint64_t blocks = want < cap ? want : cap;
  p.blocks = (uint32_t)(blocks < 1 ? 1 : blocks);
  return p;
}

#ifdef __HIPCC__
// What the select keeps on the device between its kernels, one per call
struct GrowQuantileState {
  uint32_t nleaves;
  uint32_t prefix[kGrowQuantileMaxLeaves];
  unsigned long long below[kGrowQuantileMaxLeaves];
  unsigned long long W[kGrowQuantileMaxLeaves];
  uint16_t slot_of[kGrowMaxNodes];        // a node's dense slot, kGrowQuantileNoSlot where it is no leaf
  uint16_t node_of[kGrowQuantileMaxLeaves];
};
struct GrowQuantileArgs {
  unsigned long long* hist = nullptr;     // [kGrowQuantileMaxLeaves][256] the bins of the pass at hand
  GrowQuantileState* state = nullptr;
  const uint32_t* hq = nullptr;           // [nrow] the pair plane: 0 for a row that does not count
  float alpha = 0.5f;
};
constexpr uint64_t kGrowQuantileHistBytes = (uint64_t)kGrowQuantileMaxLeaves * kGrowQuantileDigits * 8;
constexpr uint64_t kGrowQuantileBytes = kGrowQuantileHistBytes + sizeof(GrowQuantileState);

// Once per device before the first call under the quantile objective, and not before (grow.hpp grow_lds_limits_pairs)
int grow_lds_limits_quantile();
// launch_grow_tree_pairs with the quantile pair, the levels without the leaf kernel, the select over the rows as they
// stand on their leaves - per pass a memset, the pass kernel and the pick kernel, the last pick writing `value` into the
// leaves' records - and then the leaf kernel.  p.slope is alpha.  Returns a hipError_t.
int launch_grow_tree_quantile(const GrowArgs& a, const GrowPairArgs& p, const GrowQuantileArgs& q, const GrowPlan& plan,
                              const GrowPlan& levels, uint32_t round, void* stream);
// launch_grow_sse_metric, launch_grow_walk_sse_metric and launch_grow_walk_sse_deep_metric for kGrowMetricQuantile
int launch_grow_sse_quantile(const GrowEvalArgs& a, float alpha, uint32_t blocks, uint32_t t, uint32_t set, void* stream);
int launch_grow_walk_sse_quantile(const GrowEvalArgs& a, float alpha, uint32_t blocks, uint32_t round, uint32_t set, void* stream);
int launch_grow_walk_sse_deep_quantile(const GrowEvalArgs& a, const GrowDeepArgs& d, float alpha, uint32_t blocks, uint32_t round,
                                       uint32_t set, void* stream);
#endif  // __HIPCC__

}  // namespace ohx
