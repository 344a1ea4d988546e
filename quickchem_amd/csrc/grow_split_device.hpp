// Device code shared by the split kernels of boosting with row weights (grow_weighted.hip) and with row and column
// subsampling (grow_sampled.hip): the open nodes of a level, the weighted leaf record, and the two phases of the split
// choice over `ncols` histogram columns.  A column k stands for the feature map(k): the identity where every feature
// has a column, the tree's selected list where the histograms are compact.  grow_key and the cut lookup take the
// feature, the histograms and `best` the column, so the candidates and their total order are those of the header
// whichever columns are there.
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

// the open nodes of level `level`: the root alone at level 0
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

__device__ inline void grow_write_leaf_weighted(const GrowArgs& a, GrowNode* nodes, uint32_t n, int64_t G, uint64_t H,
                                                int32_t parent) {
  float leaf, weight;
  grow_solve_leaf_weighted(G, H, a.eta, a.lambda, &leaf, &weight);
  GrowNode r;
  r.G = G;
  r.H = H;
  r.left = r.right = -1;
  r.parent = parent;
  r.feature = r.cut = r.default_left = 0;
  r.value = leaf;
  r.loss_chg = 0.0f;
  r.sum_hess = (float)grow_hess(H);
  r.base_weight = weight;
  nodes[n] = r;
}

// Phase 0: a wave per (slot, column); blocks of kGrowBlock lanes over slots x ncols.  The best candidate of the column's
// feature goes to best[slot][column]; the wave of column 0 leaves the root's sums at level 0.
template <class Map>
__device__ inline void grow_split_weighted_columns(const GrowWeightedArgs& wa, uint32_t level, uint32_t round, uint32_t ncols,
                                                   Map map) {
  const GrowArgs& a = wa.g;
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t w = blockIdx.x * (kGrowBlock / kWave) + threadIdx.x / kWave;
  const uint32_t slot = w / ncols, k = w % ncols;
  if (slot >= count) return;
  const uint32_t f = map(k);
  const uint64_t at = ((uint64_t)slot * ncols + k) * kGrowBins + 4u * lane;
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
  GrowCand c = grow_best_split_weighted(g4, h4, f, 4u * lane, 4u, ncut, gi - gs, hi - hs, Gm, Hm, Gp, Hp, (double)a.lambda,
                                        wa.min_child_weight);
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const GrowCand o = grow_shuffle_cand(c, d);
    if (grow_better(o, c)) c = o;
  }
  if (lane == 0) a.best[(uint64_t)slot * ncols + k] = c;
}

// Phase 1: one block, a lane per open node.  BAG: a root that holds no weight raises kGrowFlagBag.
template <bool BAG>
__device__ inline void grow_split_weighted_nodes(const GrowWeightedArgs& wa, uint32_t level, uint32_t round, uint32_t ncols) {
  __shared__ uint32_t splits[kGrowMaxNodes / 2];
  const GrowArgs& a = wa.g;
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const uint32_t s = threadIdx.x;
  const bool active = s < count && s < kGrowMaxNodes / 2;
  const uint32_t node = begin + s;
  GrowCand best;
  int64_t Gp = 0;
  uint64_t Hp = 0;
  if (active) {
    Gp = nodes[node].G;
    Hp = nodes[node].H;
    if (level == 0) {
      grow_write_leaf_weighted(a, nodes, 0, Gp, Hp, -1);
      if (BAG && Hp == 0) atomicOr(&a.state->error, kGrowFlagBag);
    }
    for (uint32_t k = 0; k < ncols; ++k) {
      const GrowCand c = a.best[(uint64_t)s * ncols + k];
      if (grow_better(c, best)) best = c;
    }
  }
  const bool split = active && best.valid && best.loss_chg > (double)a.gamma && grow_weight_splits(Hp, wa.min_child_weight);
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
    const uint32_t f = best.key >> 9, j = (best.key >> 1) & 255u, dl = best.key & 1u;
    const uint32_t left = next + 2u * below;
    nodes[node].left = (int32_t)left;
    nodes[node].right = (int32_t)left + 1;
    nodes[node].feature = f;
    nodes[node].cut = j;
    nodes[node].default_left = dl;
    nodes[node].value = a.cuts[a.cut_ptr[f] + j];
    nodes[node].loss_chg = (float)best.loss_chg;
    grow_write_leaf_weighted(a, nodes, left, best.GL, best.HL, (int32_t)(node | 0x80000000u));
    grow_write_leaf_weighted(a, nodes, left + 1, Gp - best.GL, Hp - best.HL, (int32_t)node);
  }
  if (s == 0) {
    a.state->begin = next;
    a.state->end = next + 2u * total;
    a.state->next = next + 2u * total;
    a.tree_nodes[round] = next + 2u * total;
  }
}

}  // namespace ohx
#endif  // __HIPCC__
