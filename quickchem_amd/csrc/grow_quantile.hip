// gfx950 kernels of quantile boosting (grow_quantile.hpp; design in docs/32_quantile_objective.md).  A call runs them only
// where "ohx_objective" or "ohx_eval_metric" is quantile: with neither nothing of this file is touched, its code object
// included.
//
//   grow_pair_quantile_kernel        once per round: grow_pair_kernel's row loop with grow_pair<kGrowObjQuantile> - a
//                                    compare and a subtraction a row, no division and no square root.
//   grow_quantile_slots_kernel       once per tree, one block: the tree's leaves numbered into dense slots in node order.
//   grow_quantile_pass_kernel        four times per tree: a row whose key carries its leaf's prefix so far adds hq to
//                                    bins[slot][digit] - 64 leaves x 256 bins x 8 bytes in LDS a block, gridDim.y over the
//                                    leaf groups, 64-bit integer LDS adds, non-zero bins flushed by 64-bit global adds.  A
//                                    row is 4 bytes of hq (0: nothing else is read), 2 of pos and 8 of pred and label.
//   grow_quantile_pick_kernel        after each pass, a wave a leaf: four bins a lane, the wave's prefix sum, the first
//                                    digit at which alpha_q * W <= 2^24 * C holds; the last pick writes the leaf's value.
//   grow_sse_quantile_kernel         grow_sse_metric_kernel (grow_reg.hip) with the pinball term.
//   grow_walk_sse_quantile_kernel    grow_walk_sse_metric_kernel likewise.
//   grow_deep_walk_sse_quantile_kernel   grow_deep_walk_sse_metric_kernel likewise.
// The histogram, split, partition and leaf kernels of a quantile tree are grow_pairs.hip's and grow.hip's.  Integer adds
// only: no float atomics, no compare-and-swap loops, and the same leaves whatever the order of the rows or the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_deep_device.hpp"
#include "grow_device.hpp"
#include "grow_pairs_device.hpp"
#include "grow_quantile.hpp"
#include "grow_sums_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;
constexpr int kPassBlock = (int)kGrowHistBlock;
constexpr uint32_t kLeafBins = kGrowQuantileDigits;
static_assert(kGrowQuantileGroup * kLeafBins * 8 + 2048 <= kGrowLdsBytes, "a group's bins and the tables fit a CU's LDS");
static_assert(kGrowQuantileMaxLeaves == 1u << kGrowMaxDepth, "a tree of the deepest LDS level");
static_assert(kGrowQuantileNoSlot - kGrowQuantileMaxLeaves >= kGrowQuantileGroup, "no slot lies in no group");

// grid (blocks over the rows): grow_pair_kernel of grow_pairs.hip at the quantile objective; p.slope is alpha
__global__ __launch_bounds__(kBlock) void grow_pair_quantile_kernel(GrowArgs a, GrowPairPlanes p) {
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const float w = a.weights != nullptr ? a.weights[row] : 1.0f;
    int64_t q;
    uint32_t hq;
    flags |= grow_pair<kGrowObjQuantile>(p.slope, a.pred[row], a.labels[row], w, &q, &hq);
    if (a.bag != nullptr && !grow_row_in_bag(a.bag, row)) {   // out of the bag: its flags stay, its pair goes
      q = 0;
      hq = 0;
    }
    p.q[row] = (long long)q;
    p.hq[row] = hq;
  }
  if (flags) atomicOr(&a.state->error, flags);
}

// one block of kGrowMaxNodes lanes, a node a lane
__global__ __launch_bounds__((int)kGrowMaxNodes) void grow_quantile_slots_kernel(GrowArgs a, GrowQuantileArgs q, uint32_t round) {
  __shared__ uint32_t is_leaf[kGrowMaxNodes];
  const GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const uint32_t next = a.state->next < kGrowMaxNodes ? a.state->next : kGrowMaxNodes;
  const uint32_t i = threadIdx.x;
  const bool leaf = i < next && nodes[i].left < 0;
  is_leaf[i] = leaf ? 1u : 0u;
  __syncthreads();
  uint32_t below = 0, total = 0;
  for (uint32_t k = 0; k < next; ++k) {
    total += is_leaf[k];
    if (k < i) below += is_leaf[k];
  }
  GrowQuantileState* st = q.state;
  if (total > kGrowQuantileMaxLeaves) {   // (never: a tree of depth 8 has at most 256 leaves)
    if (i == 0) {
      atomicOr(&a.state->error, kGrowFlagState);
      st->nleaves = 0;
    }
    st->slot_of[i] = (uint16_t)kGrowQuantileNoSlot;
    return;
  }
  st->slot_of[i] = leaf ? (uint16_t)below : (uint16_t)kGrowQuantileNoSlot;
  if (leaf) {
    st->node_of[below] = (uint16_t)i;
    st->prefix[below] = 0u;
    st->below[below] = 0ull;
    st->W[below] = 0ull;
  }
  if (i == 0) st->nleaves = total;
}

// grid (blocks over the rows, leaf groups); dynamic LDS: the group's bins, kGrowQuantileGroup x 256 x 8 bytes at most
__global__ __launch_bounds__(kPassBlock) void grow_quantile_pass_kernel(GrowArgs a, GrowQuantileArgs q, uint32_t pass, uint32_t group) {
  extern __shared__ unsigned long long grow_qbins[];
  __shared__ uint16_t slot_of[kGrowMaxNodes];
  __shared__ uint32_t prefix[kGrowQuantileGroup];
  const GrowQuantileState* st = q.state;
  const uint32_t nleaves = st->nleaves;
  const uint32_t slot0 = blockIdx.y * group;
  if (slot0 >= nleaves) return;
  const uint32_t nslots = nleaves - slot0 < group ? nleaves - slot0 : group;
  const uint32_t cells = nslots * kLeafBins;
  for (uint32_t i = threadIdx.x; i < cells; i += kPassBlock) grow_qbins[i] = 0ull;
  for (uint32_t i = threadIdx.x; i < kGrowMaxNodes; i += kPassBlock) slot_of[i] = st->slot_of[i];
  for (uint32_t i = threadIdx.x; i < nslots; i += kPassBlock) prefix[i] = st->prefix[slot0 + i];
  __syncthreads();
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kPassBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kPassBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t hq = q.hq[row];
    if (hq == 0u) continue;   // out of the bag, flagged or weightless: the row does not count
    const uint32_t p = a.pos[row];
    if (p >= kGrowMaxNodes) {   // (never: the partition writes node ids)
      flags |= kGrowFlagState;
      continue;
    }
    const uint32_t s = (uint32_t)slot_of[p] - slot0;   // (a slot below slot0 wraps past nslots, and so does no slot)
    if (s >= nslots) continue;
    const uint32_t key = grow_quantile_key(a.pred[row], a.labels[row]);
    if (!grow_quantile_matches(key, prefix[s], pass)) continue;
    atomicAdd(&grow_qbins[s * kLeafBins + grow_quantile_digit(key, pass)], (unsigned long long)hq);   // s < nslots, a digit < 256
  }
  if (flags) atomicOr(&a.state->error, flags);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < cells; i += kPassBlock) {
    const unsigned long long h = grow_qbins[i];
    if (h != 0ull) atomicAdd(&q.hist[(uint64_t)slot0 * kLeafBins + i], h);   // slot0 + nslots <= nleaves <= 256
  }
}

// grid (blocks of four waves over the 256 slots), a wave a leaf
__global__ __launch_bounds__(kBlock) void grow_quantile_pick_kernel(GrowArgs a, GrowQuantileArgs q, uint32_t pass, uint32_t round) {
  GrowQuantileState* st = q.state;
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t slot = blockIdx.x * (kGrowBlock / kWave) + threadIdx.x / kWave;
  if (slot >= st->nleaves || slot >= kGrowQuantileMaxLeaves) return;
  const unsigned long long* bins = q.hist + (uint64_t)slot * kLeafBins + 4u * lane;
  unsigned long long h4[4], hs = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h4[i] = bins[i];
    hs += h4[i];
  }
  // inclusive sums across the wave (grow_split_columns' scan)
  unsigned long long hi = hs;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned long long ht = __shfl_up(hi, d, kWave);
    if (lane >= d) hi += ht;
  }
  const uint64_t total = __shfl(hi, kWave - 1, kWave);
  const uint64_t W = pass == 0 ? total : st->W[slot];
  if (pass == 0 && lane == 0) st->W[slot] = W;
  if (W == 0) return;   // a leaf without weight keeps its record
  const uint32_t alpha_q = grow_alpha_q(q.alpha);
  const uint64_t below = pass == 0 ? 0ull : st->below[slot];
  const uint32_t prefix = pass == 0 ? 0u : st->prefix[slot];
  // the lane's first bin at which the rule holds; the sums ascend, so the wave's first such lane holds the digit
  uint64_t cum = below + (hi - hs);
  int mine = -1;
  uint64_t before = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (mine < 0 && grow_quantile_reached(alpha_q, W, cum + h4[i])) {
      mine = i;
      before = cum;
    }
    cum += h4[i];
  }
  const unsigned long long found = __ballot(mine >= 0);
  if (found == 0ull) {   // (never: the bins of a pass sum to the weight of the digit picked before)
    if (lane == 0) atomicOr(&a.state->error, kGrowFlagState);
    return;
  }
  if (lane != __ffsll((long long)found) - 1) return;
  const uint32_t key = (prefix << 8) | (4u * (uint32_t)lane + (uint32_t)mine);
  st->prefix[slot] = key;
  st->below[slot] = before;
  if (pass + 1 == kGrowQuantilePasses)
    a.nodes[(uint64_t)round * kGrowMaxNodes + st->node_of[slot]].value = grow_quantile_value(key, a.eta);   // node_of < 512
}

// ---- the metric: grow_reg.hip's three kernels with the pinball term ----

// one row's hq * sq into the lane's accumulators, sq < 2^64 and hq < 2^32: the three parts of grow.hpp GrowWideSum
__device__ inline void add_weighted(unsigned long long hq, unsigned long long sq, GrowWideAcc* acc) {
  const unsigned long long ha = hq * (sq >> 32), hb = hq * (sq & kGrowLow32);   // hq, a, b < 2^32: neither product overflows
  acc->p2 += ha >> 32;
  acc->p1 += (ha & kGrowLow32) + (hb >> 32);
  acc->p0 += hb & kGrowLow32;
}

// a row of the training or the held-out set at the margin `pred`: its weight's flag, its term, its label's flag
__device__ inline void add_pinball_row(const GrowEvalArgs& a, float alpha, uint64_t row, float pred, GrowWideAcc* acc, uint32_t* flags,
                                       bool count_w) {
  float w;
  unsigned long long hq;
  if (!grow_row_weight(a.weights, row, &w, &hq)) *flags |= a.weight_flag;
  uint64_t sq;
  if (grow_metric_row<kGrowMetricQuantile>(alpha, pred, a.labels[row], &sq)) add_weighted(hq, sq, acc);
  else *flags |= a.label_flag;
  if (count_w) acc->w += hq;
}

// grid (blocks).  wslot: the set's W at t = 0, else nullptr
__global__ __launch_bounds__(kBlock) void grow_sse_quantile_kernel(GrowEvalArgs a, float alpha, unsigned long long* slot,
                                                                   unsigned long long* wslot) {
  GrowWideAcc acc;
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride)
    add_pinball_row(a, alpha, row, a.pred[row], &acc, &flags, true);
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, wslot);
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_walk_sse_quantile_kernel(GrowEvalArgs a, float alpha, uint32_t round,
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
    add_pinball_row(a, alpha, row, pred, &acc, &flags, false);
  }
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, nullptr);
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_deep_walk_sse_quantile_kernel(GrowEvalArgs a, float alpha, const EvalNode* tree,
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
      add_pinball_row(a, alpha, row, pred, &acc, &flags, false);
    }
  }
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, nullptr);
}

bool metric_args_sound(const GrowEvalArgs& a, float alpha, uint32_t blocks, uint32_t set) {
  return a.nrow != 0 && a.nrow <= kRefitMaxRows && blocks != 0 && set <= 1 && a.pred != nullptr && a.labels != nullptr &&
         a.wsums != nullptr && a.state != nullptr && grow_alpha_sound(alpha) &&
         ((a.label_flag == kGrowFlagLabel && a.weight_flag == kGrowFlagWeight) ||
          (a.label_flag == kGrowFlagEvalLabel && a.weight_flag == kGrowFlagEvalWeight));
}

}  // namespace

int grow_lds_limits_quantile() { return raise_lds_limit(grow_quantile_pass_kernel, kGrowQuantileGroup * kLeafBins * 8); }

int launch_grow_tree_quantile(const GrowArgs& a, const GrowPairArgs& p, const GrowQuantileArgs& q, const GrowPlan& plan,
                              const GrowPlan& levels, uint32_t round, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || plan.row_blocks == 0 || a.max_depth < 1 || a.max_depth > kGrowMaxDepth ||
      a.pos == nullptr || a.pred == nullptr || a.labels == nullptr || a.nodes == nullptr || a.state == nullptr || p.q == nullptr ||
      p.hq == nullptr || p.objective != kGrowObjQuantile || !grow_alpha_sound(p.slope) || q.hist == nullptr || q.state == nullptr ||
      q.hq != p.hq || q.alpha != p.slope || (a.features == nullptr && a.bag != nullptr))
    return hipErrorInvalidValue;
  GrowPairPlanes k;
  k.q = p.q;
  k.hq = p.hq;
  k.slope = p.slope;
  hipLaunchKernelGGL(grow_pair_quantile_kernel, dim3(plan.row_blocks), dim3(kBlock), 0, stream, a, k);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = (hipError_t)launch_grow_levels_pairs(a, p, plan, levels, round, stream)) != hipSuccess) return e;
  // the rows stand on their leaves; pred is the margin at the start of the round until the leaf kernel
  hipLaunchKernelGGL(grow_quantile_slots_kernel, dim3(1), dim3(kGrowMaxNodes), 0, stream, a, q, round);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const GrowQuantilePlan shape = plan_grow_quantile(a.nrow, a.max_depth, plan.row_blocks);
  const uint32_t group = shape.group, groups = shape.groups, blocks = shape.blocks;
  for (uint32_t pass = 0; pass < kGrowQuantilePasses; ++pass) {
    if ((e = hipMemsetAsync(q.hist, 0, (size_t)kGrowQuantileHistBytes, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(grow_quantile_pass_kernel, dim3(blocks, groups), dim3(kPassBlock), group * kLeafBins * 8, stream, a, q, pass, group);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(grow_quantile_pick_kernel, dim3(kGrowQuantileMaxLeaves / (kGrowBlock / kWave)), dim3(kBlock), 0, stream, a, q, pass,
                       round);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return (hipError_t)launch_grow_leaf(a, plan, round, stream);
}

int launch_grow_sse_quantile(const GrowEvalArgs& a, float alpha, uint32_t blocks, uint32_t t, uint32_t set, void* stream) {
  if (!metric_args_sound(a, alpha, blocks, set)) return hipErrorInvalidValue;
  unsigned long long* slot = a.wsums + grow_wide_index(t, set);
  unsigned long long* wslot = t == 0 ? a.wsums + set : nullptr;
  hipLaunchKernelGGL(grow_sse_quantile_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a, alpha, slot, wslot);
  return hipGetLastError();
}

int launch_grow_walk_sse_quantile(const GrowEvalArgs& a, float alpha, uint32_t blocks, uint32_t round, uint32_t set, void* stream) {
  if (!metric_args_sound(a, alpha, blocks, set) || a.bins == nullptr || a.nodes == nullptr || a.tree_nodes == nullptr ||
      a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 || a.max_depth > kGrowMaxDepth)
    return hipErrorInvalidValue;
  unsigned long long* slot = a.wsums + grow_wide_index(round + 1, set);
  hipLaunchKernelGGL(grow_walk_sse_quantile_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a, alpha, round, slot);
  return hipGetLastError();
}

int launch_grow_walk_sse_deep_quantile(const GrowEvalArgs& a, const GrowDeepArgs& d, float alpha, uint32_t blocks, uint32_t round,
                                       uint32_t set, void* stream) {
  if (!metric_args_sound(a, alpha, blocks, set) || a.bins == nullptr || a.tree_nodes == nullptr || d.eval_nodes == nullptr ||
      d.node_stride == 0 || a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 ||
      a.max_depth > kGrowDeepMaxDepth)
    return hipErrorInvalidValue;
  const hipError_t e = (hipError_t)launch_grow_deep_stage(d, blocks, round, stream);
  if (e != hipSuccess) return e;
  unsigned long long* slot = a.wsums + grow_wide_index(round + 1, set);
  hipLaunchKernelGGL(grow_deep_walk_sse_quantile_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a, alpha,
                     (const EvalNode*)d.eval_nodes, d.node_stride, round, slot);
  return hipGetLastError();
}

}  // namespace ohx
