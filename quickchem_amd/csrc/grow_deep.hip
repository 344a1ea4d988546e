// gfx950 kernels of the Deep call (grow.hpp GrowDeepArgs; design in docs/23_deep_trees.md): trees of depth 9 to 18.
// Levels 0 - 7 are the weighted call's own (launch_grow_levels_weighted); from level 8 on a level has more open nodes
// than LDS holds histograms for, so the histograms of a batch of kGrowDeepBatch node slots live in HBM.
//
//   grow_deep_widen_kernel     once per tree, after level 7: the uint16 position of a row becomes the uint32 one the
//                              deep levels use, and the uint16 one is zeroed for the next tree.
//   grow_deep_hist_kernel      once per batch: a lane takes a row in natural order; a row outside the batch leaves
//                              after the one load of its position, the others make g, w, hq and q as
//                              grow_hist_weighted_kernel does, in its order and with its flags, and add q and hq with
//                              two no-return 64-bit integer global adds a feature.  No LDS.
//   grow_deep_split_kernel<0>  once per batch: grow_split_columns with the fixed-point hessian policy over the batch's
//                              histograms; best[slot][f] is indexed by the level's slot.
//   grow_deep_split_kernel<1>  once per level, one block: the level's slots in chunks of the block's width with a
//                              running total; a lane decides its node by grow_decide_node, a ballot scan of the chunk's
//                              split flags plus the running total gives `below`, the children are grow_child_id.
//   grow_deep_partition_kernel grow_partition_kernel on the uint32 positions and the call's node stride.
//   grow_deep_leaf_kernel      grow_leaf_kernel on the same.
//   grow_deep_stage_kernel     once per round with a held-out set: the tree's GrowNodes as 16-byte EvalNodes in HBM.
//   grow_deep_walk_sse_kernel  grow_walk_sse_weighted_kernel with grow_walk_row reading that table; nothing in LDS but
//                              the reduction's partial sums.
// The Deep Sampled call (OHXBoosterBoostTreesDeepSampled; design in docs/24_deep_sampled.md) grows the same levels over a
// bag of the rows and a tree's feature list; its levels 0 - 7 are the sampled call's own (launch_grow_levels_sampled):
//   grow_deep_hist_sampled_kernel      grow_deep_hist_kernel over the bag and the list: the bag's word first, by one
//                                      scalar load a wave, then the position; the adds go to the compact
//                                      [slots][n_sel][256] histograms, the bins come from the planes of the list.
//   grow_deep_split_sampled_kernel<0>  grow_split_columns over n_sel columns and the list; the feature goes into the
//                                      key and the cut lookup.
//   grow_deep_split_sampled_kernel<1>  the chunked walk of grow_deep_split_kernel<1> (grow_deep_split_chunks, written
//                                      once) over n_sel columns.
// The widen, partition, leaf, stage and walk kernels see every row, in or out of the bag, and are the ones above.
// The level loop on the host (launch_grow_tree_deep_with) takes the launches of levels 0 - 7 and of a deep level's
// histogram as parameters: launch_grow_tree_deep gives it this file's, the pair path (grow_pairs.hip) its own.
// Only integer adds: no float atomics, no compare-and-swap loops, and the same trees and sums whatever the order of the
// rows, the batch size or the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_deep_device.hpp"
#include "grow_device.hpp"
#include "grow_sums_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

static_assert(sizeof(EvalNode) == kGrowEvalNodeBytes, "the host sizes the walk's table by it");
constexpr int kBlock = (int)kGrowBlock;
constexpr int kWaves = kBlock / kWave;

// (the tree at hand as round 0 of its own table: grow_deep_device.hpp)
__host__ __device__ inline GrowArgs tree_args(const GrowDeepArgs& a, uint32_t round) { return grow_deep_tree_args(a, round); }

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_deep_widen_kernel(GrowDeepArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.g.nrow; row += stride) {
    a.pos[row] = a.g.pos[row];
    a.g.pos[row] = 0;
  }
}

// grid (blocks).  The batch is the level's slots [batch0, batch0 + nslots); Ghist / Hhist are [nslots][F][256].
__global__ __launch_bounds__(kBlock) void grow_deep_hist_kernel(GrowDeepArgs d, uint32_t batch0, uint32_t nslots) {
  const GrowArgs& a = d.g;
  const uint32_t begin = a.state->begin, end = a.state->end;
  const uint32_t count = end - begin;
  if (batch0 >= count) return;
  const uint32_t live = count - batch0 < nslots ? count - batch0 : nslots;   // (the host's count is the device's)
  const uint32_t first = begin + batch0;
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t s = d.pos[row] - first;   // (a node below `first` wraps past live)
    if (s >= live) continue;
    const float g = a.pred[row] - a.labels[row];
    // the gradient before the weight (a NaN fails the comparison)
    if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) {
      flags |= kGrowFlagLabel;
      continue;
    }
    float w;
    unsigned long long hq;
    if (!grow_row_weight(a.weights, row, &w, &hq)) {
      flags |= kGrowFlagWeight;
      continue;
    }
    const float gw = g * w;   // one float32 multiply (-ffp-contract=off)
    if (!(__builtin_fabsf(gw) < kRefitMaxAbsGrad)) {
      flags |= kGrowFlagLabel;
      continue;
    }
    const unsigned long long q = (unsigned long long)(long long)__builtin_rintf(gw * kRefitGradScale);
    if (hq == 0ull && q == 0ull) continue;   // nothing to add
    const uint8_t* bin = a.bins + row;
    const uint64_t base = (uint64_t)s * a.num_feature * kGrowBins;
    for (uint32_t f = 0; f < a.num_feature; ++f) {
      const uint64_t i = base + (uint64_t)f * kGrowBins + bin[(uint64_t)f * a.nrow];   // s < live, f < F, bin < 256
      atomicAdd(&a.Ghist[i], q);
      atomicAdd(&a.Hhist[i], hq);
    }
  }
  if (flags) atomicOr(&a.state->error, flags);
}

// Split phase 1 of a deep level is written once, over a hessian policy, in grow_deep_device.hpp (grow_deep_split_chunks:
// its chunk loop is `for (uint32_t c0 = 0; c0 < count; c0 += kBlock)` with a running total); grow_reg.hip instantiates it too.

// PHASE 0: grid (blocks of four waves over the batch's slots x features).  PHASE 1: one block.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void grow_deep_split_kernel(GrowDeepArgs d, uint32_t level, uint32_t round, uint32_t batch0) {
  const GrowArgs a = tree_args(d, round);
  const GrowFixedHess hess{a.min_child_weight};
  if (PHASE == 0) {
    grow_split_columns(a, hess, level, 0, a.num_feature, GrowIdentityMap(), batch0);
    return;
  }
  grow_deep_split_chunks(a, hess, d.node_stride, level, a.num_feature);
}

// ---- the deep levels over a bag and a feature list ----

// A block's features, four to a 32-bit word kept in scalar registers: the packing of grow_hist_sampled_kernel, and the
// only path.  A block takes kDeepPackFeatures columns of the list and gridDim.y covers a longer one (up to four groups
// at 128 features), so the unrolled row loop keeps at most 32 plane offsets in scalar registers; a row of a second group
// reads its bag bit, position, margin, label and weight once more, which is little beside its 32 bins and 64 adds.
constexpr uint32_t kDeepPackWords = 8;
constexpr uint32_t kDeepPackFeatures = 4 * kDeepPackWords;
static_assert(kGrowMaxFeatures <= 256, "a feature is a byte");
// 64-bit words that nothing writes while the kernel runs (the bag's bit plane)
typedef const unsigned long long __attribute__((address_space(4))) * GrowConstWords;

// grid (blocks over the rows, groups of kDeepPackFeatures columns).  grow_deep_hist_kernel over the bag d.g.bag (nullptr:
// every row is in) and the n_sel features d.g.features[round][..]; Ghist / Hhist are compact, [nslots][n_sel][256].
// Eight waves a SIMD are asked for: the compiler then parks 125 scalar values (the hoisted plane offsets) in lanes of
// vector registers and reads 112 back in the row loop, never scratch.  Measured against a build without the attribute
// (seven waves, 81 lane reads in the loop) on the C360 L72 rows at depth 18, 10 rounds: 4.78 against 4.86 s at
// (0.5, 0.5) and 14.44 against 14.54 s at 26 of 27 features (docs/24_deep_sampled.md 24.4).
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
void grow_deep_hist_sampled_kernel(GrowDeepArgs d, uint32_t round, uint32_t batch0, uint32_t nslots) {
  const GrowArgs& a = d.g;
  const uint32_t begin = a.state->begin, end = a.state->end;
  const uint32_t count = end - begin;
  if (batch0 >= count) return;
  const uint32_t live = count - batch0 < nslots ? count - batch0 : nslots;   // (the host's count is the device's)
  const uint32_t first = begin + batch0;
  const uint32_t n_sel = a.n_sel;
  const uint32_t k0 = blockIdx.y * kDeepPackFeatures;   // the block's first column of the list
  if (k0 >= n_sel) return;
  const uint32_t nf = n_sel - k0 < kDeepPackFeatures ? n_sel - k0 : kDeepPackFeatures;
  // the block's features leave memory once: a byte each in wave-uniform words, so that the row loop forms a bin plane's
  // address with scalar arithmetic and loads nothing on the way to it
  const uint8_t* feat = a.features + (uint64_t)round * n_sel + k0;
  uint32_t pack[kDeepPackWords];
#pragma unroll
  for (uint32_t j = 0; j < kDeepPackWords; ++j) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)   // (a byte past the last feature repeats the word's first: see the row loop)
      if (4 * j < nf) v |= (uint32_t)feat[4 * j + b < nf ? 4 * j + b : 4 * j] << (8 * b);
    pack[j] = __builtin_amdgcn_readfirstlane(v);
  }
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    if (a.bag != nullptr) {
      // A wave's 64 rows share one word of the plane: a block starts at a multiple of kBlock, a wave at a multiple of 64
      // within it, and the stride is a multiple of kBlock, so the wave's first row is a multiple of 64 on every trip and
      // its lanes are the 64 rows after it (those below nrow).  rows < 2^31, so the word index fits 32 bits.
      // The plane is written by grow_bag_kernel before this kernel starts and by nothing while it runs; the kernel's own
      // global adds keep the compiler from proving that, so the word is read through the constant address space, which
      // says so and makes the read the scalar load it is in grow_hist_sampled_kernel.
      const uint32_t word = __builtin_amdgcn_readfirstlane((uint32_t)(row >> 6));
      const unsigned long long bits = ((GrowConstWords)a.bag)[word];
      if (((bits >> (row & 63u)) & 1ull) == 0ull) continue;   // out of the bag: nothing else is read
    }
    const uint32_t s = d.pos[row] - first;   // (a node below `first` wraps past live)
    if (s >= live) continue;
    const float g = a.pred[row] - a.labels[row];
    // the gradient before the weight (a NaN fails the comparison)
    if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) {
      flags |= kGrowFlagLabel;
      continue;
    }
    float w;
    unsigned long long hq;
    if (!grow_row_weight(a.weights, row, &w, &hq)) {
      flags |= kGrowFlagWeight;
      continue;
    }
    const float gw = g * w;   // one float32 multiply (-ffp-contract=off)
    if (!(__builtin_fabsf(gw) < kRefitMaxAbsGrad)) {
      flags |= kGrowFlagLabel;
      continue;
    }
    const unsigned long long q = (unsigned long long)(long long)__builtin_rintf(gw * kRefitGradScale);
    if (hq == 0ull && q == 0ull) continue;   // nothing to add
    const uint8_t* bins = a.bins + row;
    const uint64_t base = ((uint64_t)s * n_sel + k0) * kGrowBins;   // s < live <= nslots, k0 + k < n_sel, a bin is a byte
    unsigned long long* G = a.Ghist + base;
    unsigned long long* H = a.Hhist + base;
    // a word's four bin loads leave together, then their adds: the lane waits for memory once a word, not once a
    // feature.  A byte past the block's last feature repeats the word's first feature: its load reads the address the
    // first load reads, and is not used.
#pragma unroll
    for (uint32_t j = 0; j < kDeepPackWords; ++j) {
      if (4 * j >= nf) break;
      const uint32_t p = pack[j];
      const uint32_t b0 = bins[(uint64_t)(p & 255u) * a.nrow], b1 = bins[(uint64_t)((p >> 8) & 255u) * a.nrow];
      const uint32_t b2 = bins[(uint64_t)((p >> 16) & 255u) * a.nrow], b3 = bins[(uint64_t)(p >> 24) * a.nrow];
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
  if (flags) atomicOr(&a.state->error, flags);
}

// PHASE 0: grid (blocks of four waves over the batch's slots x n_sel).  PHASE 1: one block.  (kGrowFlagBag is raised by
// the sampled phase 1 at level 0, which is never a deep level.)
template <int PHASE>
__global__ __launch_bounds__(kBlock) void grow_deep_split_sampled_kernel(GrowDeepArgs d, uint32_t level, uint32_t round,
                                                                         uint32_t batch0) {
  const GrowArgs a = tree_args(d, round);
  const GrowFixedHess hess{a.min_child_weight};
  if (PHASE == 0) {
    GrowListMap map;
    map.list = a.features + (uint64_t)round * a.n_sel;
    grow_split_columns(a, hess, level, 0, a.n_sel, map, batch0);
    return;
  }
  grow_deep_split_chunks(a, hess, d.node_stride, level, a.n_sel);
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_deep_partition_kernel(GrowDeepArgs d, uint32_t round) {
  const GrowArgs& a = d.g;
  const GrowNode* nodes = a.nodes + (uint64_t)round * d.node_stride;
  const uint32_t next = a.state->next;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t p = d.pos[row];
    if (p >= next || p >= d.node_stride) {
      atomicOr(&a.state->error, kGrowFlagState);
      continue;
    }
    const int32_t left = nodes[p].left;
    if (left < 0) continue;
    const uint32_t f = nodes[p].feature;
    if (f >= a.num_feature) {
      atomicOr(&a.state->error, kGrowFlagState);
      continue;
    }
    const uint32_t b = a.bins[(uint64_t)f * a.nrow + row];
    const bool go_left = b == kGrowMissingBin ? nodes[p].default_left != 0u : b <= nodes[p].cut;
    d.pos[row] = (uint32_t)(go_left ? left : nodes[p].right);
  }
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_deep_leaf_kernel(GrowDeepArgs d, uint32_t round) {
  const GrowArgs& a = d.g;
  const GrowNode* nodes = a.nodes + (uint64_t)round * d.node_stride;
  const uint32_t next = a.state->next;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t p = d.pos[row];
    if (p < next && p < d.node_stride) a.pred[row] += nodes[p].value;
    else atomicOr(&a.state->error, kGrowFlagState);
    d.pos[row] = 0;
  }
}

// ---- the held-out walk ----

// grid (blocks).  The count is checked by the walk kernel; here it only bounds the copy.
__global__ __launch_bounds__(kBlock) void grow_deep_stage_kernel(GrowDeepArgs d, uint32_t round) {
  const GrowNode* nodes = d.g.nodes + (uint64_t)round * d.node_stride;
  uint32_t count = d.g.tree_nodes[round];
  if (count > d.node_stride) count = d.node_stride;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) static_cast<EvalNode*>(d.eval_nodes)[i] = grow_eval_node(nodes[i]);
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_deep_walk_sse_kernel(GrowEvalArgs a, const EvalNode* tree, uint32_t node_stride,
                                                                    uint32_t round, unsigned long long* slot) {
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
      float w;
      unsigned long long hq;
      if (!grow_row_weight(a.weights, row, &w, &hq)) flags |= a.weight_flag;
      if (!grow_add_weighted_square(pred, a.labels[row], hq, &acc)) flags |= a.label_flag;
    }
  }
  if (flags) atomicOr(&a.state->error, flags);
  grow_reduce_wide(acc, slot, nullptr);
}

// the histogram columns of a tree: the tree's feature list where the call has one, else every feature
uint32_t deep_columns(const GrowArgs& a) { return a.features != nullptr ? a.n_sel : a.num_feature; }

// ncols: the histogram columns of the deep levels, the tree's or fewer (GrowDeepLaunches::ncols)
bool deep_args_sound(const GrowDeepArgs& d, const GrowDeepPlan& plan, uint32_t ncols) {
  const GrowArgs& a = d.g;
  if (ncols > deep_columns(a)) return false;
  return a.nrow != 0 && a.nrow <= kRefitMaxRows && a.num_feature != 0 && a.num_feature <= kGrowMaxFeatures && ncols != 0 &&
         ncols <= a.num_feature && (a.features != nullptr || a.bag == nullptr) &&
         a.max_depth > kGrowMaxDepth && a.max_depth <= kGrowDeepMaxDepth && a.min_child_weight >= 0.0 && d.pos != nullptr &&
         d.node_stride != 0 && (uint64_t)d.node_stride == grow_deep_node_stride(a.nrow, a.max_depth) &&
         plan.node_stride == d.node_stride && plan.batch != 0 && plan.hist_blocks != 0 && plan.lds.row_blocks != 0 &&
         plan.lds.levels.size() == (size_t)kGrowMaxDepth &&
         plan.scratch_bytes == std::min<uint64_t>(plan.batch, grow_deep_max_open(a.nrow, a.max_depth)) * ncols * kGrowBins * 16;
}

}  // namespace

// The inline path's launches: the gradient is made in the histogram kernels, from pred, label and weight.
int launch_grow_tree_deep(const GrowDeepArgs& d, const GrowDeepPlan& plan, uint32_t round, GrowLevelState* h_state, void* stream_) {
  GrowDeepLaunches l;
  // levels 0 - 7: the weighted call's kernels, or the sampled call's over the bag and the tree's list
  l.top = [](const GrowArgs& top, const GrowPlan& lds, void* s) {
    return top.features != nullptr ? launch_grow_levels_sampled(top, lds, lds, 0, s) : launch_grow_levels_weighted(top, lds, lds, 0, s);
  };
  l.hist = [](const GrowDeepArgs& a, uint32_t, uint32_t r, uint32_t batch0, uint32_t nslots, uint32_t hist_blocks, void* s) {
    hipStream_t stream = static_cast<hipStream_t>(s);
    if (a.g.features != nullptr)
      hipLaunchKernelGGL(grow_deep_hist_sampled_kernel, dim3(hist_blocks, (a.g.n_sel + kDeepPackFeatures - 1) / kDeepPackFeatures),
                         dim3(kBlock), 0, stream, a, r, batch0, nslots);
    else hipLaunchKernelGGL(grow_deep_hist_kernel, dim3(hist_blocks), dim3(kBlock), 0, stream, a, batch0, nslots);
  };
  return launch_grow_tree_deep_with(d, plan, round, h_state, stream_, l);
}

int launch_grow_tree_deep_with(const GrowDeepArgs& d, const GrowDeepPlan& plan, uint32_t round, GrowLevelState* h_state,
                               void* stream_, const GrowDeepLaunches& launches) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const uint32_t ncols = launches.ncols != 0 ? launches.ncols : deep_columns(d.g);
  if (!deep_args_sound(d, plan, ncols) || h_state == nullptr || !launches.top || !launches.hist) return hipErrorInvalidValue;
  // levels 0 - 7 on the tree's own records (a tree of 8 levels has at most 511 of them, and no more than 2 * nrow - 1:
  // within the stride either way)
  const bool sampled = d.g.features != nullptr;
  GrowArgs top = tree_args(d, round);
  top.max_depth = kGrowMaxDepth;
  if (sampled) top.features += (uint64_t)round * deep_columns(d.g);   // round 0 of its own list, as of its own records
  hipError_t e = (hipError_t)launches.top(top, plan.lds, stream);
  if (e != hipSuccess) return e;
  // the level word after phase 1 of level d - 1: the open nodes of level d
  auto level_word = [&]() {
    hipError_t r = hipMemcpyAsync(h_state, d.g.state, sizeof(GrowLevelState), hipMemcpyDeviceToHost, stream);
    return r != hipSuccess ? r : hipStreamSynchronize(stream);
  };
  if ((e = level_word()) != hipSuccess) return e;
  uint32_t count = h_state->end - h_state->begin;
  if (count == 0 || h_state->error != 0) return (hipError_t)launch_grow_leaf(top, plan.lds, 0, stream);
  const dim3 rows(plan.lds.row_blocks), block(kBlock);
  hipLaunchKernelGGL(grow_deep_widen_kernel, rows, block, 0, stream, d);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint64_t max_open = grow_deep_max_open(d.g.nrow, d.g.max_depth);
  for (uint32_t level = kGrowMaxDepth; level < (uint32_t)d.g.max_depth && count != 0 && h_state->error == 0; ++level) {
    if (count > max_open) return hipErrorInvalidValue;   // (never: `best` holds max_open slots)
    for (uint32_t batch0 = 0; batch0 < count; batch0 += plan.batch) {
      const uint32_t nslots = std::min(plan.batch, count - batch0);
      const size_t bytes = (size_t)nslots * ncols * kGrowBins * sizeof(unsigned long long);
      if ((e = hipMemsetAsync(d.g.Ghist, 0, bytes, stream)) != hipSuccess) return e;
      if ((e = hipMemsetAsync(d.g.Hhist, 0, bytes, stream)) != hipSuccess) return e;
      launches.hist(d, level, round, batch0, nslots, plan.hist_blocks, stream);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      const dim3 waves((nslots * ncols + kWaves - 1) / kWaves);
      if (launches.split0) launches.split0(d, level, round, batch0, waves.x, stream);
      else if (sampled) hipLaunchKernelGGL(grow_deep_split_sampled_kernel<0>, waves, block, 0, stream, d, level, round, batch0);
      else hipLaunchKernelGGL(grow_deep_split_kernel<0>, waves, block, 0, stream, d, level, round, batch0);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (launches.split1) launches.split1(d, level, round, stream);
    else if (sampled) hipLaunchKernelGGL(grow_deep_split_sampled_kernel<1>, dim3(1), block, 0, stream, d, level, round, 0u);
    else hipLaunchKernelGGL(grow_deep_split_kernel<1>, dim3(1), block, 0, stream, d, level, round, 0u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(grow_deep_partition_kernel, rows, block, 0, stream, d, round);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (level + 1 == (uint32_t)d.g.max_depth) break;   // the last level: nothing follows that needs the count
    if ((e = level_word()) != hipSuccess) return e;
    count = h_state->end - h_state->begin;
  }
  hipLaunchKernelGGL(grow_deep_leaf_kernel, rows, block, 0, stream, d, round);
  return hipGetLastError();
}

int launch_grow_deep_stage(const GrowDeepArgs& d, uint32_t blocks, uint32_t round, void* stream_) {
  if (blocks == 0 || d.eval_nodes == nullptr || d.node_stride == 0 || d.g.nodes == nullptr || d.g.tree_nodes == nullptr)
    return hipErrorInvalidValue;
  const uint32_t stage_blocks = std::min<uint32_t>(blocks, (d.node_stride + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(grow_deep_stage_kernel, dim3(stage_blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream_), d, round);
  return hipGetLastError();
}

int launch_grow_walk_sse_deep(const GrowEvalArgs& a, const GrowDeepArgs& d, uint32_t blocks, uint32_t round, uint32_t set,
                              void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || blocks == 0 || set > 1 || a.pred == nullptr || a.labels == nullptr ||
      a.wsums == nullptr || a.state == nullptr || a.bins == nullptr || a.tree_nodes == nullptr || d.eval_nodes == nullptr ||
      d.node_stride == 0 || a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 ||
      a.max_depth > kGrowDeepMaxDepth ||
      !((a.label_flag == kGrowFlagLabel && a.weight_flag == kGrowFlagWeight) ||
        (a.label_flag == kGrowFlagEvalLabel && a.weight_flag == kGrowFlagEvalWeight)))
    return hipErrorInvalidValue;
  const uint32_t stage_blocks = std::min<uint32_t>(blocks, (d.node_stride + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(grow_deep_stage_kernel, dim3(stage_blocks), dim3(kBlock), 0, stream, d, round);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grow_deep_walk_sse_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, (const EvalNode*)d.eval_nodes,
                     d.node_stride, round, a.wsums + grow_wide_index(round + 1, set));
  return hipGetLastError();
}

}  // namespace ohx
