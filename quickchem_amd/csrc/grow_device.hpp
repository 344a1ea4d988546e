// What the kernel files of the tree grower share (grow.hip, grow_eval.hip and the two files for row weights and for
// subsampling), each written once: the open nodes of a level, the shuffle of a candidate, the leaf record, the two
// phases of the split choice, the held-out rows' walk of one tree, and the level loop on the host.
//
// The split phases take a hessian policy (grow.hpp: GrowCountHess or GrowFixedHess) and work over `ncols` histogram
// columns.  A column k stands for the feature map(k): the identity where every feature has a column, the tree's
// selected list where the histograms are compact.  grow_key and the cut lookup take the feature, the histograms and
// `best` the column, so the candidates and their total order are those of grow.hpp whichever columns are there.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "walk_device.hpp"

namespace ohx {

// column k is feature k
struct GrowIdentityMap {
  __device__ uint32_t operator()(uint32_t k) const { return k; }
};
// column k is feature list[k] (ascending)
struct GrowListMap {
  const uint8_t* list;
  __device__ uint32_t operator()(uint32_t k) const { return list[k]; }
};

// the open nodes of level `level`: the root alone at level 0, whatever the state word still holds from the last tree
__device__ inline void grow_level_range(const GrowArgs& a, uint32_t level, uint32_t* begin, uint32_t* end, uint32_t* next) {
  if (level == 0) {
    *begin = 0;
    *end = 1;
    *next = 1;
  } else {
    *begin = a.state->begin;
    *end = a.state->end;
    *next = a.state->next;
  }
}

__device__ inline GrowCand grow_shuffle_cand(const GrowCand& c, int d) {
  GrowCand o;
  o.loss_chg = __shfl_xor(c.loss_chg, d, kWave);
  o.GL = __shfl_xor((long long)c.GL, d, kWave);
  o.HL = __shfl_xor((unsigned long long)c.HL, d, kWave);
  o.key = __shfl_xor(c.key, d, kWave);
  o.valid = __shfl_xor(c.valid, d, kWave);
  return o;
}

template <class Hess>
__device__ inline void grow_write_leaf(const GrowArgs& a, const Hess& hess, GrowNode* nodes, uint32_t n, int64_t G, uint64_t H,
                                       int32_t parent) {
  float leaf, weight;
  hess.solve_leaf(G, H, a.eta, a.lambda, &leaf, &weight);
  GrowNode r;
  r.G = G;
  r.H = H;
  r.left = r.right = -1;
  r.parent = parent;
  r.feature = r.cut = r.default_left = 0;
  r.value = leaf;
  r.loss_chg = 0.0f;
  r.sum_hess = hess.sum_hess(H);
  r.base_weight = weight;
  nodes[n] = r;
}

// Phase 0: a wave per (slot, column); blocks of kGrowBlock lanes over slots x ncols - integer prefix sums across the 256
// bins, the shared gain in double, and a butterfly reduction by the total order of grow_better.  The best candidate of
// the column's feature goes to best[slot][column]; the wave of column 0 leaves the root's sums at level 0.  The
// histograms hold the slots from slot0 on (a batch of the level: grow_deep.hip); `best` is indexed by the level's slot.
template <class Hess, class Map>
__device__ inline void grow_split_columns(const GrowArgs& a, const Hess& hess, uint32_t level, uint32_t round, uint32_t ncols,
                                          Map map, uint32_t slot0 = 0) {
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t w = blockIdx.x * (kGrowBlock / kWave) + threadIdx.x / kWave;
  const uint32_t local = w / ncols, k = w % ncols;
  const uint32_t slot = slot0 + local;
  if (slot >= count) return;
  const uint32_t f = map(k);
  const uint64_t at = ((uint64_t)local * ncols + k) * kGrowBins + 4u * lane;
  int64_t g4[4];
  uint64_t h4[4];
  int64_t gs = 0;
  uint64_t hs = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    g4[i] = (int64_t)a.Ghist[at + i];
    h4[i] = (uint64_t)a.Hhist[at + i];
    gs += g4[i];
    hs += h4[i];
  }
  // inclusive sums across the wave, then the sums below the lane's first bin
  long long gi = gs;
  unsigned long long hi = hs;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const long long gt = __shfl_up(gi, d, kWave);
    const unsigned long long ht = __shfl_up(hi, d, kWave);
    if (lane >= d) {
      gi += gt;
      hi += ht;
    }
  }
  const int64_t Gp = __shfl(gi, kWave - 1, kWave);
  const uint64_t Hp = __shfl(hi, kWave - 1, kWave);
  const int64_t Gm = __shfl((long long)g4[3], kWave - 1, kWave);
  const uint64_t Hm = __shfl((unsigned long long)h4[3], kWave - 1, kWave);
  if (level == 0 && k == 0 && lane == 0) {   // the root's sums: every row that adds is in one bin of column 0
    nodes[0].G = Gp;
    nodes[0].H = Hp;
  }
  const uint32_t ncut = a.cut_ptr[f + 1] - a.cut_ptr[f];
  GrowCand c = grow_best_split<Hess>(g4, h4, f, 4u * lane, 4u, ncut, gi - gs, hi - hs, Gm, Hm, Gp, Hp, (double)a.lambda, hess);
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const GrowCand o = grow_shuffle_cand(c, d);
    if (grow_better(o, c)) c = o;
  }
  if (lane == 0) a.best[(uint64_t)slot * ncols + k] = c;
}

// The decision of one open node, written once for both phase-1 kernels: its sums, the best of its columns
// (best[slot][0 .. ncols), ascending, replaced by a strictly better one only), and whether it splits.  At level 0 the
// root's record is written as a leaf first.  BAG: a root that holds no weight raises kGrowFlagBag.
struct GrowDecision {
  GrowCand best;
  int64_t Gp = 0;
  uint64_t Hp = 0;
  bool split = false;
};
template <bool BAG, class Hess>
__device__ inline GrowDecision grow_decide_node(const GrowArgs& a, const Hess& hess, GrowNode* nodes, uint32_t level,
                                                uint32_t node, uint32_t slot, uint32_t ncols) {
  GrowDecision d;
  d.Gp = nodes[node].G;
  d.Hp = nodes[node].H;
  if (level == 0) {
    grow_write_leaf(a, hess, nodes, 0, d.Gp, d.Hp, -1);
    if (BAG && d.Hp == 0) atomicOr(&a.state->error, kGrowFlagBag);
  }
  for (uint32_t k = 0; k < ncols; ++k) {
    const GrowCand c = a.best[(uint64_t)slot * ncols + k];
    if (grow_better(c, d.best)) d.best = c;
  }
  d.split = d.best.valid && d.best.loss_chg > (double)a.gamma && hess.evaluates(d.Hp);
  return d;
}
// The records of a node that splits into `left` and left + 1: its own fields and both children as leaves.
template <class Hess>
__device__ inline void grow_write_split(const GrowArgs& a, const Hess& hess, GrowNode* nodes, uint32_t node,
                                        const GrowDecision& d, uint32_t left) {
  const uint32_t f = d.best.key >> 9, j = (d.best.key >> 1) & 255u, dl = d.best.key & 1u;
  nodes[node].left = (int32_t)left;
  nodes[node].right = (int32_t)left + 1;
  nodes[node].feature = f;
  nodes[node].cut = j;
  nodes[node].default_left = dl;
  nodes[node].value = a.cuts[a.cut_ptr[f] + j];
  nodes[node].loss_chg = (float)d.best.loss_chg;
  grow_write_leaf(a, hess, nodes, left, d.best.GL, d.best.HL, (int32_t)(node | 0x80000000u));
  grow_write_leaf(a, hess, nodes, left + 1, d.Gp - d.best.GL, d.Hp - d.best.HL, (int32_t)node);
}

// Phase 1: one block, a lane per open node takes the best of its columns, the splitting nodes get their child ids in
// ascending node order, the records are written.
template <bool BAG, class Hess>
__device__ inline void grow_split_nodes(const GrowArgs& a, const Hess& hess, uint32_t level, uint32_t round, uint32_t ncols) {
  __shared__ uint32_t splits[kGrowMaxNodes / 2];
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const uint32_t s = threadIdx.x;
  const bool active = s < count && s < kGrowMaxNodes / 2;
  const uint32_t node = begin + s;
  GrowDecision d;
  if (active) d = grow_decide_node<BAG>(a, hess, nodes, level, node, s, ncols);
  const bool split = active && d.split;
  if (s < kGrowMaxNodes / 2) splits[s] = split ? 1u : 0u;
  __syncthreads();
  uint32_t below = 0, total = 0;
  const uint32_t live = count < kGrowMaxNodes / 2 ? count : kGrowMaxNodes / 2;
  for (uint32_t i = 0; i < live; ++i) {
    total += splits[i];
    if (i < s) below += splits[i];
  }
  if (next + 2u * total > kGrowMaxNodes) {   // (never: a tree of depth 8 has 511 nodes)
    if (s == 0) atomicOr(&a.state->error, kGrowFlagState);
    total = 0;
  } else if (split) {
    grow_write_split(a, hess, nodes, node, d, next + 2u * below);
  }
  if (s == 0) {
    a.state->begin = next;
    a.state->end = next + 2u * total;
    a.state->next = next + 2u * total;
    a.tree_nodes[round] = next + 2u * total;
  }
}

// ---- the held-out rows' walk of one tree (the metric's walk kernels) ----

// a node as the walk needs it
struct EvalNode {
  int32_t left, right;   // -1: a leaf
  uint32_t fcd;          // feature << 9 | cut << 1 | default_left
  float value;           // the leaf value
};
static_assert(sizeof(EvalNode) == 16, "16 bytes a node");
__device__ inline EvalNode grow_eval_node(const GrowNode& n) {
  EvalNode e;
  e.left = n.left;
  e.right = n.right;
  e.fcd = (n.feature << 9) | ((n.cut & 255u) << 1) | (n.default_left != 0u ? 1u : 0u);
  e.value = n.value;
  return e;
}

// The block stages the records of tree `round` in tree[kGrowMaxNodes] (LDS) and meets at a barrier.  Returns the
// tree's nodes, or 0 where the count is unsound: the error word is raised, no barrier is met, and the block ends.
__device__ inline uint32_t grow_stage_tree(const GrowEvalArgs& a, uint32_t round, EvalNode* tree) {
  const uint32_t count = a.tree_nodes[round];
  if (count == 0 || count > kGrowMaxNodes) {   // (never: the split kernel writes it, and refuses a 513th node itself)
    if (threadIdx.x == 0) atomicOr(&a.state->error, kGrowFlagState);
    return 0;
  }
  const GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  for (uint32_t i = threadIdx.x; i < count; i += kGrowBlock) tree[i] = grow_eval_node(nodes[i]);
  __syncthreads();
  return count;
}

// A row walks the staged tree from the root by its bin planes, as grow_partition_kernel steps.  True and the leaf's
// index; false where a feature or a child lies outside its table or no leaf is met within max_depth steps.
__device__ inline bool grow_walk_row(const GrowEvalArgs& a, const EvalNode* tree, uint32_t count, uint64_t row, uint32_t* leaf) {
  uint32_t p = 0;
  for (int d = 0; d < a.max_depth; ++d) {
    const EvalNode e = tree[p];
    if (e.left < 0) break;
    const uint32_t f = e.fcd >> 9;
    if (f >= a.num_feature) return false;
    const uint32_t b = a.bins[(uint64_t)f * a.nrow + row];
    const bool go_left = b == kGrowMissingBin ? (e.fcd & 1u) != 0u : b <= ((e.fcd >> 1) & 255u);
    p = (uint32_t)(go_left ? e.left : e.right);
    if (p >= count) return false;
  }
  *leaf = p;
  return tree[p].left < 0;   // (tree[p] is read only while p < count)
}

// ---- the level loop (host) ----

// One tree, round `round`: the soundness of the arguments and of the level plan, then per level the two histogram
// memsets, the histogram kernel, both split phases and the partition kernel, and the leaf kernel at the end.  Each kernel
// file instantiates it with its own three launches (hist takes the level's plan and the level; split0 the blocks and the
// level; split1 the level) over `ncols` histogram columns of pair_bytes a (node, column) pair in LDS.  max_trips bounds
// the trips of a histogram block over the rows where its LDS hessian is a 32-bit count (grow_hist_kernel:
// kGrowMaxTrips); 0 where it is a 64-bit sum, which 2^31 rows cannot overflow.  leaf == false leaves the rows standing on
// their nodes after the last level's partition: the caller goes on from there (the deep levels of grow_deep.hip).
template <class Hist, class Split0, class Split1>
inline hipError_t grow_launch_tree(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round,
                                   hipStream_t stream, uint32_t ncols, uint32_t pair_bytes, uint64_t max_trips, Hist hist,
                                   Split0 split0, Split1 split1, bool leaf = true) {
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 ||
      a.max_depth > kGrowMaxDepth || levels.levels.size() != (size_t)a.max_depth || plan.row_blocks == 0 || ncols == 0 ||
      ncols > a.num_feature)
    return hipErrorInvalidValue;
  const uint32_t max_pairs = kGrowLdsBytes / pair_bytes;
  hipError_t e = hipSuccess;
  for (uint32_t d = 0; d < (uint32_t)a.max_depth; ++d) {
    const GrowLevelPlan& l = levels.levels[d];
    if (l.slots != (1u << d) || l.node_group * l.feat_group > max_pairs || l.node_group == 0 || l.feat_group == 0 ||
        l.lds_bytes != l.node_group * l.feat_group * pair_bytes || l.node_groups * l.node_group < l.slots ||
        l.feat_groups * l.feat_group < ncols || l.hist_blocks == 0)
      return hipErrorInvalidValue;
    const uint64_t per_trip = (uint64_t)l.hist_blocks * kGrowHistBlock;
    if (max_trips != 0 && (a.nrow + per_trip - 1) / per_trip > max_trips) return hipErrorInvalidValue;
    const size_t bytes = (size_t)l.slots * ncols * kGrowBins * sizeof(unsigned long long);
    if ((e = hipMemsetAsync(a.Ghist, 0, bytes, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.Hhist, 0, bytes, stream)) != hipSuccess) return e;
    hist(l, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t waves = l.slots * ncols, per_block = kGrowBlock / kWave;
    split0((waves + per_block - 1) / per_block, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    split1(d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = (hipError_t)launch_grow_partition(a, plan, round, stream)) != hipSuccess) return e;
  }
  return leaf ? (hipError_t)launch_grow_leaf(a, plan, round, stream) : hipSuccess;
}

}  // namespace ohx
#endif  // __HIPCC__
