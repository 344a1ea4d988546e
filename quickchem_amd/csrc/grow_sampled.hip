// gfx950 kernels of boosting with row and column subsampling (grow.hpp GrowArgs; design in docs/22_sampling.md).
//
//   grow_bag_kernel               once per tree: a lane takes a row and evaluates the draw (grow_in_bag); the wave's 64
//                                 results become one 64-bit word of the bit plane bag[ceil(nrow / 64)], written by one
//                                 lane.  The rows past nrow in the last word are 0.
//   grow_hist_sampled_kernel      once per level: grow_hist_weighted_kernel over the tree's selected features - the
//                                 block's feature group indexes features[round][0 .. n_sel), its bin planes are
//                                 bins + features[k] * nrow, and the global histograms are compact [slots][n_sel][256].
//                                 A lane whose bit of the plane is clear goes on before it reads pred, label or weight.
//                                 The block's features sit four to a word in scalar registers, and a word's four bin
//                                 loads are in flight together.
//   grow_split_sampled_kernel<0>  grow_device.hpp's phase 0 over n_sel columns; the feature goes into the key and
//                                 the cut lookup.
//   grow_split_sampled_kernel<1>  its phase 1; a root without weight raises kGrowFlagBag.
// The partition, leaf and metric kernels see every row and are those of the weighted call (launch_grow_partition,
// launch_grow_leaf, launch_grow_sse_weighted, launch_grow_walk_sse_weighted).  Only integer adds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "grow_device.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;
constexpr int kHistBlock = (int)kGrowHistBlock;
// a block's features, four to a 32-bit word kept in scalar registers; a word's four bin loads are in flight together
constexpr uint32_t kPackWords = (kGrowWeightedMaxPairs + 3) / 4;
static_assert(kGrowMaxFeatures <= 256, "a feature is a byte");

// grid (blocks over the words x 64 rows).  A wave's rows are one word: the block's first row and the stride are
// multiples of 64, and the loop's bound is too, so all 64 lanes take every trip together.
__global__ __launch_bounds__(kBlock) void grow_bag_kernel(GrowArgs a) {
  const uint64_t nrow = a.nrow;
  const uint64_t padded = ((nrow + 63) / 64) * 64;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < padded; row += stride) {
    const bool in = row < nrow && grow_in_bag(a.row_key, row, a.k_s);
    const unsigned long long word = __ballot(in);
    if ((threadIdx.x & (kWave - 1)) == 0) a.bag[row >> 6] = word;
  }
}

// grid (blocks over the rows, node groups x feature groups); dynamic LDS: node_group x feat_group x 256 x (8 + 8).
// The unrolled row loop keeps up to 40 plane offsets in scalar registers; eight waves a SIMD (two blocks a CU where LDS
// allows) are asked for, so the compiler parks what does not fit 96 of them in lanes of a vector register, never scratch.
__global__ __launch_bounds__(kHistBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void grow_hist_sampled_kernel(GrowArgs a, uint32_t level, uint32_t round,
                                                                       uint32_t node_group, uint32_t feat_group,
                                                                       uint32_t feat_groups) {
  extern __shared__ unsigned long long grow_shist[];
  uint32_t begin, end, next;
  grow_level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  const uint32_t slot0 = (blockIdx.y / feat_groups) * node_group;
  const uint32_t k0 = (blockIdx.y % feat_groups) * feat_group;   // the block's first column of the selected list
  if (slot0 >= count || k0 >= a.n_sel) return;
  const uint32_t nslots = count - slot0 < node_group ? count - slot0 : node_group;
  const uint32_t nf = a.n_sel - k0 < feat_group ? a.n_sel - k0 : feat_group;
  // the block's features leave memory once: a byte each in wave-uniform words, so that the row loop forms a bin plane's
  // address with scalar arithmetic and loads nothing on the way to it
  const uint8_t* feat = a.features + (uint64_t)round * a.n_sel + k0;
  uint32_t pack[kPackWords];
#pragma unroll
  for (uint32_t j = 0; j < kPackWords; ++j) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)   // (a byte past the last feature repeats the word's first: see the row loop)
      if (4 * j < nf) v |= (uint32_t)feat[4 * j + b < nf ? 4 * j + b : 4 * j] << (8 * b);
    pack[j] = __builtin_amdgcn_readfirstlane(v);
  }
  const uint32_t cells = node_group * feat_group * kGrowBins;
  unsigned long long* Gl = grow_shist;
  unsigned long long* Hl = grow_shist + cells;
  for (uint32_t i = threadIdx.x; i < 2u * cells; i += kHistBlock) grow_shist[i] = 0ull;
  __syncthreads();
  const uint32_t first = begin + slot0;
  uint32_t flags = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kHistBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kHistBlock + threadIdx.x; row < a.nrow; row += stride) {
    if (a.bag != nullptr) {
      // the wave's rows share one word (the first row of a wave and the stride are multiples of 64; rows < 2^31)
      const uint32_t word = __builtin_amdgcn_readfirstlane((uint32_t)(row >> 6));
      if (((a.bag[word] >> (row & 63u)) & 1ull) == 0ull) continue;
    }
    const uint32_t s = (uint32_t)a.pos[row] - first;   // (a node below `first` wraps past nslots)
    if (s >= nslots) continue;
    const float g = a.pred[row] - a.labels[row];
    // the gradient before the weight (a NaN fails the comparison)
    if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) {
      flags |= kGrowFlagLabel;
      continue;
    }
    const float w = a.weights != nullptr ? a.weights[row] : 1.0f;
    if (!grow_weight_sound(w)) {
      flags |= kGrowFlagWeight;
      continue;
    }
    const unsigned long long hq = (unsigned long long)__builtin_rintf(w * kRefitGradScale);   // < 2^32
    const float gw = g * w;   // one float32 multiply (-ffp-contract=off)
    if (!(__builtin_fabsf(gw) < kRefitMaxAbsGrad)) {
      flags |= kGrowFlagLabel;
      continue;
    }
    const unsigned long long q = (unsigned long long)(long long)__builtin_rintf(gw * kRefitGradScale);
    if (hq == 0ull && q == 0ull) continue;   // nothing to add
    const uint8_t* bins = a.bins + row;
    const uint32_t base = s * feat_group * kGrowBins;
    // a word's four bin loads leave together, then their adds: the lane waits for memory once a word, not once a
    // feature.  A byte past the block's last feature repeats the word's first feature: its load reads the address the
    // first load reads, and is not used.
#pragma unroll
    for (uint32_t j = 0; j < kPackWords; ++j) {
      if (4 * j >= nf) break;
      const uint32_t p = pack[j];
      const uint32_t b0 = bins[(uint64_t)(p & 255u) * a.nrow], b1 = bins[(uint64_t)((p >> 8) & 255u) * a.nrow];
      const uint32_t b2 = bins[(uint64_t)((p >> 16) & 255u) * a.nrow], b3 = bins[(uint64_t)(p >> 24) * a.nrow];
      const uint32_t at = base + 4 * j * kGrowBins;
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
  if (flags) atomicOr(&a.state->error, flags);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < cells; i += kHistBlock) {
    const unsigned long long g = Gl[i], h = Hl[i];
    if ((g | h) == 0ull) continue;
    const uint32_t s = i / (feat_group * kGrowBins), k = (i / kGrowBins) % feat_group, b = i % kGrowBins;
    if (s >= nslots || k >= nf) continue;
    const uint64_t gi = ((uint64_t)(slot0 + s) * a.n_sel + k0 + k) * kGrowBins + b;
    if (h != 0ull) atomicAdd(&a.Hhist[gi], h);
    if (g != 0ull) atomicAdd(&a.Ghist[gi], g);
  }
}

// PHASE 0: grid (blocks of four waves over slots x n_sel).  PHASE 1: one block.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void grow_split_sampled_kernel(GrowArgs a, uint32_t level, uint32_t round) {
  const GrowFixedHess hess{a.min_child_weight};
  if (PHASE == 0) {
    GrowListMap map;
    map.list = a.features + (uint64_t)round * a.n_sel;
    grow_split_columns(a, hess, level, round, a.n_sel, map);
  } else {
    grow_split_nodes<true>(a, hess, level, round, a.n_sel);
  }
}

bool sampled_args_sound(const GrowArgs& a) {
  return a.nrow != 0 && a.nrow <= kRefitMaxRows && a.num_feature != 0 && a.num_feature <= kGrowMaxFeatures && a.n_sel != 0 &&
         a.n_sel <= a.num_feature && a.k_s != 0 && a.k_s <= kGrowSampleOne;
}

}  // namespace

int grow_lds_limits_sampled() {
  return raise_lds_limit(grow_hist_sampled_kernel, kGrowWeightedMaxPairs * kGrowWeightedPairBytes);
}

int launch_grow_bag(const GrowArgs& a, const GrowPlan& plan, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!sampled_args_sound(a) || a.bag == nullptr || plan.row_blocks == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_bag_kernel, dim3(plan.row_blocks), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

namespace {

hipError_t sampled_levels(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, hipStream_t stream,
                          bool leaf) {
  if (!sampled_args_sound(a) || a.features == nullptr || !(a.min_child_weight >= 0.0)) return hipErrorInvalidValue;
  return grow_launch_tree(
      a, plan, levels, round, stream, a.n_sel, kGrowWeightedPairBytes, 0,
      [&](const GrowLevelPlan& l, uint32_t d) {
        hipLaunchKernelGGL(grow_hist_sampled_kernel, dim3(l.hist_blocks, l.node_groups * l.feat_groups), dim3(kHistBlock),
                           l.lds_bytes, stream, a, d, round, l.node_group, l.feat_group, l.feat_groups);
      },
      [&](uint32_t blocks, uint32_t d) {
        hipLaunchKernelGGL(grow_split_sampled_kernel<0>, dim3(blocks), dim3(kBlock), 0, stream, a, d, round);
      },
      [&](uint32_t d) { hipLaunchKernelGGL(grow_split_sampled_kernel<1>, dim3(1), dim3(kBlock), 0, stream, a, d, round); }, leaf);
}

}  // namespace

int launch_grow_tree_sampled(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream) {
  return sampled_levels(a, plan, levels, round, static_cast<hipStream_t>(stream), true);
}

int launch_grow_levels_sampled(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream) {
  return sampled_levels(a, plan, levels, round, static_cast<hipStream_t>(stream), false);
}

}  // namespace ohx
