// gfx950 kernels of boosters with categorical splits (categorical.hpp; design in docs/14_categorical.md).
//
// One lane owns one row, a wave 64 rows (consecutive ones, or a brick of the caller's grid).  A node is 16 bytes (flatten.hpp CatNode) and is fetched with ONE
// 128-bit gather per step: a divergent wave64 gather costs the texture addresser the same for 4, 8 or 16 bytes
// (docs/04_tree_walk_cost.md), so the set of a categorical node rides in the node's value word where it fits (largest
// category < 32) and only larger sets cost a second, single-word gather - issued under the exec mask of the lanes
// that stand on such a node with a value inside the set's capacity.
//
// Routing at a categorical node (include/ohxgb.h):  missing -> default child;  v < 0 or v >= size -> default child;
// otherwise bit (int)v of the set: set -> right, clear -> left.  Missing is NaN here (canonicalised at the fill, or as
// the row is read), and NaN fails 0 <= v < size, so the first two cases are one comparison.  The cast is only made
// for a value inside [0, size), size <= 2**24: no float outside int range is ever cast.
//
// No atomics on the output and no cross-lane arithmetic: a row's bits depend on the row, the trees and `missing` only.
// The tile and the direct kernel evaluate the same expressions in the same order and agree bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "categorical.hpp"
#include "kernels.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr size_t kCuLdsBytes = 160 * 1024;
// trees a lane of the tile kernel walks at once: that many dependent gathers in flight per lane
#ifndef OHX_CAT_CHAINS
#define OHX_CAT_CHAINS 2
#endif
constexpr int kChains = OHX_CAT_CHAINS;

// The child a row with value v (NaN = missing) takes at node nd: 0 = left, 1 = right.
__device__ __forceinline__ uint32_t step_right(const uint4& nd, float v, const uint32_t* __restrict__ words) {
  const bool dl = (nd.z >> 31) != 0u;
  const bool is_cat = (nd.z & kCatFlag) != 0u;
  // numeric: missing -> default, else v < cond -> left
  const bool num_left = (v != v) ? dl : (v < __uint_as_float(nd.x));
  // categorical: a category only inside [0, size); NaN is outside
  const bool in_range = is_cat && v >= 0.0f && v < __uint_as_float(nd.w);
  const uint32_t c = in_range ? (uint32_t)(int32_t)v : 0u;
  uint32_t word = nd.x;
  if (in_range && (nd.z & kCatWords) != 0u) word = words[nd.x + (c >> 5)];
  const bool cat_left = in_range ? ((word >> (c & 31u)) & 1u) == 0u : dl;
  return (is_cat ? cat_left : num_left) ? 0u : 1u;
}

// Margins: the wave's rows staged once in LDS as tile[feature * 64 + lane] (conflict-free: bank = lane % 32 whatever
// the feature), every tree of the range walked two at a time so that two dependent gathers are in flight per lane,
// the leaves added in tree order.
__global__ __launch_bounds__(kBlock) void predict_cat_tile_kernel(DeviceCatForest fr, CatPredictArgs a) {
  extern __shared__ float cat_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  float* tile = cat_lds + (size_t)wave * fr.num_feature * kWave + lane;
  const __amdgpu_buffer_rsrc_t nodes = make_rsrc(fr.nodes, fr.node_bytes);
  const uint32_t* __restrict__ words = fr.words;
  const bool missing_is_nan = a.missing != a.missing;
  const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t t64 = (uint64_t)blockIdx.x * kWavesPerBlock + wave; t64 < a.ntiles; t64 += nwaves) {
    bool valid;
    const uint64_t row = tile_row(a.shape, t64, lane, a.nrow, &valid);
    if (!__any(valid)) continue;                 // a brick that overhangs the rows altogether
    (void)stage_rows<true>(tile, a.rows, row, valid, a.ncol, fr.num_feature, a.missing, missing_is_nan, a.flags);
    // (a wave reads only its own tile, each lane only its own column: no barrier)
    float acc = fr.base_score;
    uint32_t t = a.tree_begin;
    for (; t + kChains <= a.tree_end; t += kChains) {
      uint4 n[kChains];
#pragma unroll
      for (int c = 0; c < kChains; ++c) n[c] = load_node16(nodes, fr.roots[t + c]);
      bool walking = true;
      while (walking) {
        walking = false;
#pragma unroll
        for (int c = 0; c < kChains; ++c) {
          if (n[c].y != 0u) n[c] = load_node16(nodes, n[c].y + step_right(n[c], tile[(n[c].z & kCatFeatureMask) * kWave], words));
          walking |= n[c].y != 0u;
        }
      }
#pragma unroll
      for (int c = 0; c < kChains; ++c) acc += __uint_as_float(n[c].x);      // in tree order
    }
    for (; t < a.tree_end; ++t) {
      uint4 n0 = load_node16(nodes, fr.roots[t]);
      while (n0.y != 0u) n0 = load_node16(nodes, n0.y + step_right(n0, tile[(n0.z & kCatFeatureMask) * kWave], words));
      acc += __uint_as_float(n0.x);
    }
    if (valid) a.out[row] = acc;
  }
}

// Any feature count, no LDS: every lane reads its own row from global memory.  Margins, or (PRED_LEAF) the node id
// of every tree's leaf as a float, [nrow][ntree].
template <bool PRED_LEAF>
__global__ __launch_bounds__(kBlock) void predict_cat_direct_kernel(DeviceCatForest fr, CatPredictArgs a) {
  const __amdgpu_buffer_rsrc_t nodes = make_rsrc(fr.nodes, fr.node_bytes);
  const uint32_t* __restrict__ words = fr.words;
  const bool missing_is_nan = a.missing != a.missing;
  const float qnan = __builtin_nanf("");
  const uint32_t ntree = a.tree_end - a.tree_begin;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < a.nrow; row += stride) {
    const float* x = a.rows + row * (uint64_t)a.ncol;
    // +-inf anywhere in the row, walked or not: what the tile kernel's fill sees
    bool any_inf = false;
    for (uint32_t f = 0; f < a.ncol; ++f) any_inf |= is_inf(x[f]);
    if (any_inf && !is_inf(a.missing) && a.flags) atomicOr(a.flags, kFlagInfInput);
    float acc = fr.base_score;
    for (uint32_t t = a.tree_begin; t < a.tree_end; ++t) {
      uint32_t slot = fr.roots[t];
      uint4 nd = load_node16(nodes, slot);
      while (nd.y != 0u) {
        const uint32_t f = nd.z & kCatFeatureMask;
        float v = qnan;
        if (f < a.ncol) {
          v = x[f];
          if (!missing_is_nan && v == a.missing) v = qnan;
        }
        slot = nd.y + step_right(nd, v, words);
        nd = load_node16(nodes, slot);
      }
      if (PRED_LEAF) a.out[row * (uint64_t)ntree + (t - a.tree_begin)] = (float)fr.orig_id[slot];
      else acc += __uint_as_float(nd.x);
    }
    if (!PRED_LEAF) a.out[row] = acc;
  }
}

size_t cat_tile_lds_bytes(uint32_t num_feature) { return (size_t)kWavesPerBlock * num_feature * kWave * sizeof(float); }

}  // namespace

bool cat_uses_tile(uint32_t num_feature, bool pred_leaf, bool force_direct) {
  return !pred_leaf && !force_direct && num_feature != 0 && cat_tile_lds_bytes(num_feature) <= kCuLdsBytes;
}

const char* cat_kernel_symbol(uint32_t num_feature, bool pred_leaf, bool force_direct) {
  if (cat_uses_tile(num_feature, pred_leaf, force_direct)) return "predict_cat_tile_kernel";
  return pred_leaf ? "predict_cat_direct_kernel<true>" : "predict_cat_direct_kernel<false>";
}

hipError_t launch_predict_cat(const DeviceCatForest& fr, const CatPredictArgs& args, int num_cus, bool force_direct,
                              hipStream_t stream, const LaunchTuning& tune) {
  CatPredictArgs a = args;
  a.shape = pick_shape_dense(tune, a.nrow);
  a.ntiles = a.shape.ntiles(a.nrow);
  if (a.nrow == 0 || (a.pred_leaf && a.tree_end == a.tree_begin)) return hipSuccess;
  if (a.tree_end < a.tree_begin || a.tree_end > fr.num_trees || a.ncol > fr.num_feature) return hipErrorInvalidValue;
  if (cat_uses_tile(fr.num_feature, a.pred_leaf, force_direct)) {
    const size_t lds = cat_tile_lds_bytes(fr.num_feature);
    const hipError_t e = raise_lds_limit(predict_cat_tile_kernel, lds);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, predict_cat_tile_kernel, kBlock, lds) != hipSuccess || per_cu < 1)
      per_cu = 1;
    uint64_t blocks = (a.ntiles + kWavesPerBlock - 1) / kWavesPerBlock;
    const uint64_t cap = (uint64_t)num_cus * (uint64_t)per_cu;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(predict_cat_tile_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, stream, fr, a);
    return hipGetLastError();
  }
  uint64_t blocks = (a.nrow + kBlock - 1) / kBlock;
  const uint64_t cap = (uint64_t)num_cus * 8u;
  if (blocks > cap) blocks = cap;
  if (a.pred_leaf) hipLaunchKernelGGL(predict_cat_direct_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, fr, a);
  else hipLaunchKernelGGL(predict_cat_direct_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, fr, a);
  return hipGetLastError();
}

}  // namespace ohx
