// gfx950 kernels of the pair path of boosting (grow.hpp GrowPairArgs; design in docs/26_objectives.md): a round's
// (gradient, hessian) pair of every row is made once, by the call's objective, and the histogram kernels add what they
// read.
//
//   grow_pair_kernel<OBJ>            once per round: one streaming pass over the rows - pred, label, weight and, with a
//                                    bag, the bag's word (a scalar load a wave) in; q (int64) and hq (uint32) out, 12
//                                    bytes a row.  grow.hpp's grow_pair<OBJ> makes the pair and the flags of every row,
//                                    in or out of the bag; a row out of the bag or with a flag has the pair (0, 0).
//                                    OBJ is a template argument: squared error divides nothing.
//   grow_hist_pairs_kernel           once per level to 7: grow_hist_sampled_kernel's structure over a feature list (the
//                                    identity list where the call samples no columns) - the LDS histogram of a node
//                                    group x feature group, two 64-bit integer LDS adds a feature, flushed with 64-bit
//                                    global adds.  It computes no gradient and checks nothing: a row is its bag bit, its
//                                    position and its pair, and a row whose pair is (0, 0) adds nothing.
//   grow_deep_hist_pairs_kernel      once per batch of a level from 8 on: grow_deep_hist_sampled_kernel's structure - a
//                                    row a lane, packed feature bytes in wave-uniform registers, two no-return 64-bit
//                                    integer global adds a feature.  No LDS.
//   grow_split_pairs_kernel<0, ..>   grow_device.hpp's phase 0 with the fixed-point hessian policy over the list.
//   grow_split_pairs_kernel<1, ROOT> its phase 1.  ROOT says what a root without hessian (H == 0) raises at level 0:
//                                    nothing (the weighted call), kGrowFlagBag (the sampled call at squared error) or
//                                    kGrowFlagHess (pseudo-Huber, with or without a bag).
// Both histogram kernels keep the wave-uniform early exit on the bag's word: it costs one scalar load a wave and spares a
// row out of the bag the 2 or 4 bytes of its position and the 12 of its pair, which at subsample 0.5 is half the
// histogram kernels' row traffic; the zero pair alone would read them all.  The zero pair still skips the rows the word
// cannot know about: a weight of 0 and a gradient that rounds to 0.
// The split phases of the deep levels, and the partition, leaf, widen, stage, walk and metric kernels read no gradient
// and are the inline path's own.  Only integer adds: no float atomics, no compare-and-swap loops, and the same trees
// whatever the order of the rows or the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_device.hpp"
#include "grow_pairs_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;
constexpr int kHistBlock = (int)kGrowHistBlock;
// the LDS levels: a block's features, four to a 32-bit word kept in scalar registers (grow_hist_sampled_kernel's packing)
constexpr uint32_t kPackWords = (kGrowWeightedMaxPairs + 3) / 4;
// the deep levels: a block takes 32 columns of the list and gridDim.y covers a longer one (grow_deep_hist_sampled_kernel)
constexpr uint32_t kDeepPackWords = 8;
constexpr uint32_t kDeepPackFeatures = 4 * kDeepPackWords;
static_assert(kGrowMaxFeatures <= 256, "a feature is a byte");
enum : int { kRootNone = 0, kRootBag = 1, kRootHess = 2 };
static_assert(kRootNone == kGrowRootNone && kRootBag == kGrowRootBag && kRootHess == kGrowRootHess, "grow.hpp names them for the host");

// grid (blocks over the rows).  A block's first row and the stride are multiples of 64, so a wave's rows share one word
// of the bag.  24 bytes a row with weights (20 without), and an eighth of a byte with a bag.
template <uint32_t OBJ>
__global__ __launch_bounds__(kBlock) void grow_pair_kernel(GrowArgs a, GrowPairPlanes p) {
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const float w = a.weights != nullptr ? a.weights[row] : 1.0f;
    int64_t q;
    uint32_t hq;
    flags |= grow_pair<OBJ>(p.slope, a.pred[row], a.labels[row], w, &q, &hq);
    if (a.bag != nullptr && !grow_row_in_bag(a.bag, row)) {   // out of the bag: its flags stay, its pair goes
      q = 0;
      hq = 0;
    }
    p.q[row] = (long long)q;
    p.hq[row] = hq;
  }
  if (flags) atomicOr(&a.state->error, flags);
}

// grid (blocks over the rows, node groups x feature groups); dynamic LDS: node_group x feat_group x 256 x (8 + 8).
// Eight waves a SIMD are asked for, as grow_hist_sampled_kernel asks: scalar values that do not fit are parked in lanes of
// a vector register, never scratch.
__global__ __launch_bounds__(kHistBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
void grow_hist_pairs_kernel(GrowArgs a, GrowPairPlanes p, uint32_t level, uint32_t node_group, uint32_t feat_group, uint32_t feat_groups) {
  extern __shared__ unsigned long long grow_phist[];
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  const uint32_t slot0 = (blockIdx.y / feat_groups) * node_group;
  const uint32_t k0 = (blockIdx.y % feat_groups) * feat_group;   // the block's first column of the list
  if (slot0 >= count || k0 >= p.ncols) return;
  const uint32_t nslots = count - slot0 < node_group ? count - slot0 : node_group;
  const uint32_t nf = p.ncols - k0 < feat_group ? p.ncols - k0 : feat_group;
  uint32_t pack[kPackWords];
  grow_pack_features<kPackWords>(p.list + k0, nf, pack);
  const uint32_t cells = node_group * feat_group * kGrowBins;
  unsigned long long* Gl = grow_phist;
  unsigned long long* Hl = grow_phist + cells;
  for (uint32_t i = threadIdx.x; i < 2u * cells; i += kHistBlock) grow_phist[i] = 0ull;
  __syncthreads();
  const uint32_t first = begin + slot0;
  const uint64_t stride = (uint64_t)gridDim.x * kHistBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kHistBlock + threadIdx.x; row < a.nrow; row += stride) {
    if (a.bag != nullptr && !grow_row_in_bag(a.bag, row)) continue;   // out of the bag: nothing else is read
    const uint32_t s = (uint32_t)a.pos[row] - first;   // (a node below `first` wraps past nslots)
    if (s >= nslots) continue;
    unsigned long long q, hq;
    if (!grow_load_pair(p, row, &q, &hq)) continue;   // nothing to add
    const uint8_t* bins = a.bins + row;
    const uint32_t base = s * feat_group * kGrowBins;
    // a word's four bin loads leave together, then their adds: the lane waits for memory once a word
#pragma unroll
    for (uint32_t j = 0; j < kPackWords; ++j) {
      if (4 * j >= nf) break;
      const uint32_t w = pack[j];
      const uint32_t b0 = bins[(uint64_t)(w & 255u) * a.nrow], b1 = bins[(uint64_t)((w >> 8) & 255u) * a.nrow];
      const uint32_t b2 = bins[(uint64_t)((w >> 16) & 255u) * a.nrow], b3 = bins[(uint64_t)(w >> 24) * a.nrow];
      const uint32_t at = base + 4 * j * kGrowBins;   // s < nslots <= node_group, 4 j + 3 < feat_group x 4 / 4 rounded up
      atomicAdd(&Gl[at + b0], q);
      atomicAdd(&Hl[at + b0], hq);
      if (4 * j + 1 < nf) {
        atomicAdd(&Gl[at + kGrowBins + b1], q);
        atomicAdd(&Hl[at + kGrowBins + b1], hq);
      }
      if (4 * j + 2 < nf) {
        atomicAdd(&Gl[at + 2 * kGrowBins + b2], q);
        atomicAdd(&Hl[at + 2 * kGrowBins + b2], hq);
      }
      if (4 * j + 3 < nf) {
        atomicAdd(&Gl[at + 3 * kGrowBins + b3], q);
        atomicAdd(&Hl[at + 3 * kGrowBins + b3], hq);
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < cells; i += kHistBlock) {
    const unsigned long long g = Gl[i], h = Hl[i];
    if ((g | h) == 0ull) continue;
    const uint32_t s = i / (feat_group * kGrowBins), k = (i / kGrowBins) % feat_group, b = i % kGrowBins;
    if (s >= nslots || k >= nf) continue;
    const uint64_t gi = ((uint64_t)(slot0 + s) * p.ncols + k0 + k) * kGrowBins + b;
    if (h != 0ull) atomicAdd(&a.Hhist[gi], h);
    if (g != 0ull) atomicAdd(&a.Ghist[gi], g);
  }
}

// grid (blocks over the rows, groups of kDeepPackFeatures columns).  The batch is the level's slots [batch0, batch0 +
// nslots); Ghist / Hhist are compact, [nslots][ncols][256].
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
void grow_deep_hist_pairs_kernel(GrowDeepArgs d, GrowPairPlanes p, uint32_t batch0, uint32_t nslots) {
  const GrowArgs& a = d.g;
  const uint32_t begin = a.state->begin, end = a.state->end;
  const uint32_t count = end - begin;
  if (batch0 >= count) return;
  const uint32_t live = count - batch0 < nslots ? count - batch0 : nslots;   // (the host's count is the device's)
  const uint32_t first = begin + batch0;
  const uint32_t ncols = p.ncols;
  const uint32_t k0 = blockIdx.y * kDeepPackFeatures;   // the block's first column of the list
  if (k0 >= ncols) return;
  const uint32_t nf = ncols - k0 < kDeepPackFeatures ? ncols - k0 : kDeepPackFeatures;
  uint32_t pack[kDeepPackWords];
  grow_pack_features<kDeepPackWords>(p.list + k0, nf, pack);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    if (a.bag != nullptr && !grow_row_in_bag(a.bag, row)) continue;   // out of the bag: nothing else is read
    const uint32_t s = d.pos[row] - first;   // (a node below `first` wraps past live)
    if (s >= live) continue;
    unsigned long long q, hq;
    if (!grow_load_pair(p, row, &q, &hq)) continue;   // nothing to add
    const uint8_t* bins = a.bins + row;
    const uint64_t base = ((uint64_t)s * ncols + k0) * kGrowBins;   // s < live <= nslots, k0 + k < ncols, a bin is a byte
    unsigned long long* G = a.Ghist + base;
    unsigned long long* H = a.Hhist + base;
#pragma unroll
    for (uint32_t j = 0; j < kDeepPackWords; ++j) {
      if (4 * j >= nf) break;
      const uint32_t w = pack[j];
      const uint32_t b0 = bins[(uint64_t)(w & 255u) * a.nrow], b1 = bins[(uint64_t)((w >> 8) & 255u) * a.nrow];
      const uint32_t b2 = bins[(uint64_t)((w >> 16) & 255u) * a.nrow], b3 = bins[(uint64_t)(w >> 24) * a.nrow];
      const uint32_t at = 4 * j * kGrowBins;
      atomicAdd(&G[at + b0], q);
      atomicAdd(&H[at + b0], hq);
      if (4 * j + 1 < nf) {
        atomicAdd(&G[at + kGrowBins + b1], q);
        atomicAdd(&H[at + kGrowBins + b1], hq);
      }
      if (4 * j + 2 < nf) {
        atomicAdd(&G[at + 2 * kGrowBins + b2], q);
        atomicAdd(&H[at + 2 * kGrowBins + b2], hq);
      }
      if (4 * j + 3 < nf) {
        atomicAdd(&G[at + 3 * kGrowBins + b3], q);
        atomicAdd(&H[at + 3 * kGrowBins + b3], hq);
      }
    }
  }
}

// PHASE 0: grid (blocks of four waves over slots x columns).  PHASE 1: one block.  The bodies are grow_device.hpp's, with
// the fixed-point hessian sum and the list's columns.
template <int PHASE, int ROOT>
__global__ __launch_bounds__(kBlock) void grow_split_pairs_kernel(GrowArgs a, GrowPairPlanes p, uint32_t level, uint32_t round) {
  const GrowFixedHess hess{a.min_child_weight};
  if (PHASE == 0) {
    GrowListMap map;
    map.list = p.list;
    grow_split_columns(a, hess, level, round, p.ncols, map);
  } else {
    grow_split_nodes<ROOT == kRootBag>(a, hess, level, round, p.ncols);
    // the root's sums are phase 0's, written before this kernel started
    if (ROOT == kRootHess && level == 0 && threadIdx.x == 0 && a.nodes[(uint64_t)round * kGrowMaxNodes].H == 0)
      atomicOr(&a.state->error, kGrowFlagHess);
  }
}

bool pairs_args_sound(const GrowArgs& a, const GrowPairArgs& p) {
  return a.nrow != 0 && a.nrow <= kRefitMaxRows && a.num_feature != 0 && a.num_feature <= kGrowMaxFeatures && p.q != nullptr &&
         p.hq != nullptr && p.identity != nullptr && a.pred != nullptr && a.labels != nullptr && a.state != nullptr &&
         (p.objective == kGrowObjSquared || (p.objective == kGrowObjPseudoHuber && grow_slope_sound(p.slope)) ||
          (p.objective == kGrowObjQuantile && grow_alpha_sound(p.slope))) &&
         (a.features != nullptr ? a.n_sel != 0 && a.n_sel <= a.num_feature && a.k_s != 0 && a.k_s <= kGrowSampleOne
                                : a.bag == nullptr) &&
         a.min_child_weight >= 0.0;
}

// the planes and the columns of one tree: `list` is the tree's own list, or nullptr for every feature
GrowPairPlanes planes_of(const GrowArgs& a, const GrowPairArgs& p, const uint8_t* list) {
  GrowPairPlanes k;
  k.q = p.q;
  k.hq = p.hq;
  k.list = list != nullptr ? list : p.identity;
  k.ncols = list != nullptr ? a.n_sel : a.num_feature;
  k.slope = p.slope;
  return k;
}

hipError_t launch_pair_kernel(const GrowArgs& a, const GrowPairArgs& p, const GrowPairPlanes& k, const GrowPlan& plan, hipStream_t stream) {
  if (plan.row_blocks == 0) return hipErrorInvalidValue;
  if (p.objective == kGrowObjPseudoHuber)
    hipLaunchKernelGGL(grow_pair_kernel<kGrowObjPseudoHuber>, dim3(plan.row_blocks), dim3(kBlock), 0, stream, a, k);
  else hipLaunchKernelGGL(grow_pair_kernel<kGrowObjSquared>, dim3(plan.row_blocks), dim3(kBlock), 0, stream, a, k);
  return hipGetLastError();
}

// The pair kernel (make_pairs; without, the planes hold the round's pairs already: grow_quantile.hip makes its own), then
// grow_device.hpp's level loop with this file's launches.  `list`: the tree's own list or nullptr.
// `tree`: the call's round, which `round` is not where the tree is round 0 of its own table; it picks the lists of a
// column-sampled call (splits->levels), whose level d adds and splits the columns of its own list.
hipError_t pairs_levels(const GrowArgs& a, const GrowPairArgs& p, const uint8_t* list, const GrowPlan& plan, const GrowPlan& levels,
                        uint32_t round, uint32_t tree, hipStream_t stream, bool leaf, const GrowPairSplits* splits,
                        bool make_pairs = true) {
  if (!pairs_args_sound(a, p) || (make_pairs && p.objective == kGrowObjQuantile)) return hipErrorInvalidValue;
  const bool by_level = splits != nullptr && splits->levels.lists != nullptr;
  if (by_level ? !splits->level_split0 || !splits->level_split1 || splits->levels.depth < (uint32_t)a.max_depth ||
                     splits->levels.n_lvl == 0 || splits->levels.n_lvl > (list != nullptr ? a.n_sel : a.num_feature)
               : splits != nullptr && (!splits->split0 || !splits->split1))
    return hipErrorInvalidValue;
  const GrowPairPlanes k = planes_of(a, p, list);
  // the planes and the columns of level d
  auto planes_at = [&](uint32_t d) {
    GrowPairPlanes kd = k;
    if (by_level) {
      kd.list = splits->levels.list(tree, d);
      kd.ncols = splits->levels.n_lvl;
    }
    return kd;
  };
  if (make_pairs) {
    const hipError_t e = launch_pair_kernel(a, p, k, plan, stream);
    if (e != hipSuccess) return e;
  }
  const int root = p.objective == kGrowObjPseudoHuber ? kRootHess : list != nullptr ? kRootBag : kRootNone;
  return grow_launch_tree(
      a, plan, levels, round, stream, planes_at(0).ncols, kGrowWeightedPairBytes, 0,
      [&](const GrowLevelPlan& l, uint32_t d) {
        hipLaunchKernelGGL(grow_hist_pairs_kernel, dim3(l.hist_blocks, l.node_groups * l.feat_groups), dim3(kHistBlock), l.lds_bytes,
                           stream, a, planes_at(d), d, l.node_group, l.feat_group, l.feat_groups);
      },
      [&](uint32_t blocks, uint32_t d) {
        if (by_level) return splits->level_split0(a, tree, blocks, d, round, stream);
        if (splits != nullptr) return splits->split0(a, k.list, k.ncols, blocks, d, round, stream);
        hipLaunchKernelGGL((grow_split_pairs_kernel<0, kRootNone>), dim3(blocks), dim3(kBlock), 0, stream, a, k, d, round);
      },
      [&](uint32_t d) {
        if (by_level) return splits->level_split1(a, tree, root, d, round, stream);
        if (splits != nullptr) return splits->split1(a, k.list, k.ncols, root, d, round, stream);
        if (root == kRootHess) hipLaunchKernelGGL((grow_split_pairs_kernel<1, kRootHess>), dim3(1), dim3(kBlock), 0, stream, a, k, d, round);
        else if (root == kRootBag) hipLaunchKernelGGL((grow_split_pairs_kernel<1, kRootBag>), dim3(1), dim3(kBlock), 0, stream, a, k, d, round);
        else hipLaunchKernelGGL((grow_split_pairs_kernel<1, kRootNone>), dim3(1), dim3(kBlock), 0, stream, a, k, d, round);
      },
      leaf);
}

}  // namespace

int grow_lds_limits_pairs() { return raise_lds_limit(grow_hist_pairs_kernel, kGrowWeightedMaxPairs * kGrowWeightedPairBytes); }

int launch_grow_tree_pairs(const GrowArgs& a, const GrowPairArgs& p, const GrowPlan& plan, const GrowPlan& levels, uint32_t round,
                           void* stream, const GrowPairSplits* splits) {
  const uint8_t* list = a.features != nullptr ? a.features + (uint64_t)round * a.n_sel : nullptr;
  return pairs_levels(a, p, list, plan, levels, round, round, static_cast<hipStream_t>(stream), true, splits);
}

int launch_grow_levels_pairs(const GrowArgs& a, const GrowPairArgs& p, const GrowPlan& plan, const GrowPlan& levels, uint32_t round,
                             void* stream) {
  const uint8_t* list = a.features != nullptr ? a.features + (uint64_t)round * a.n_sel : nullptr;
  return pairs_levels(a, p, list, plan, levels, round, round, static_cast<hipStream_t>(stream), false, nullptr, false);
}

int launch_grow_tree_deep_pairs(const GrowDeepArgs& d, const GrowPairArgs& p, const GrowDeepPlan& plan, uint32_t round,
                                GrowLevelState* h_state, void* stream, const GrowPairSplits* splits) {
  if (!pairs_args_sound(d.g, p)) return hipErrorInvalidValue;
  if (splits != nullptr && (!splits->deep_split0 || !splits->deep_split1)) return hipErrorInvalidValue;
  GrowDeepLaunches l;
  if (splits != nullptr) {
    l.split0 = splits->deep_split0;
    l.split1 = splits->deep_split1;
  }
  // (top.features is the tree's own list already: round 0 of its own list, as of its own records)
  const bool by_level = splits != nullptr && splits->levels.lists != nullptr;
  if (by_level && (splits->levels.depth < (uint32_t)d.g.max_depth || splits->levels.n_lvl == 0 ||
                   splits->levels.n_lvl > (d.g.features != nullptr ? d.g.n_sel : d.g.num_feature)))
    return hipErrorInvalidValue;
  if (by_level) l.ncols = splits->levels.n_lvl;
  l.top = [&p, splits, round](const GrowArgs& top, const GrowPlan& lds, void* s) {
    return (int)pairs_levels(top, p, top.features, lds, lds, 0, round, static_cast<hipStream_t>(s), false, splits);
  };
  l.hist = [&p, splits, by_level](const GrowDeepArgs& a, uint32_t level, uint32_t r, uint32_t batch0, uint32_t nslots, uint32_t hist_blocks,
                                  void* s) {
    GrowPairPlanes k = planes_of(a.g, p, a.g.features != nullptr ? a.g.features + (uint64_t)r * a.g.n_sel : nullptr);
    if (by_level) {   // the level's own list
      k.list = splits->levels.list(r, level);
      k.ncols = splits->levels.n_lvl;
    }
    hipLaunchKernelGGL(grow_deep_hist_pairs_kernel, dim3(hist_blocks, (k.ncols + kDeepPackFeatures - 1) / kDeepPackFeatures),
                       dim3(kBlock), 0, static_cast<hipStream_t>(s), a, k, batch0, nslots);
  };
  return launch_grow_tree_deep_with(d, plan, round, h_state, stream, l);
}

}  // namespace ohx
