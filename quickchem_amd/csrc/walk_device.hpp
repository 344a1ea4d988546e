// Device routines every row-tile walk shares (kernels.hip, categorical.hip, visits.hip, refit.hip): which row a lane
// takes, how a wave's rows reach LDS, how a node is fetched, the walk to a dense leaf index and the per-leaf add.
// For hipcc translation units only; everything is inlined into the kernels of the file that includes it.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"   // TileShape, kFlagInfInput

namespace ohx {

constexpr int kWave = 64;

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool is_inf(float v) { return __builtin_isinf(v); }

// ------------------------------------------------------------------ node loads

// Nodes are read through a buffer descriptor: one 64- or 128-bit load per node that the compiler cannot split into
// narrower loads (it does split a plain uint2 or uint4 load whose words are used at different points, which multiplies
// the gathers), a 32-bit offset instead of a 64-bit address, and a hardware range check that turns a stray slot into a
// read of zeros - whose child word is 0, a leaf (of value 0, of dense index 0) - instead of a fault.  Whoever emits a
// node array keeps it under 4 GiB.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint2 load_node8(__amdgpu_buffer_rsrc_t r, uint32_t slot) {
  const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)(slot << 3), 0, 0);
  return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint4 load_node16(__amdgpu_buffer_rsrc_t r, uint32_t slot) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(slot << 4), 0, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// ------------------------------------------------------------------ lanes -> rows

// Row of this lane in tile `tile_id` (TileShape, kernels.hpp): without a grid tile t is rows 64 t .. 64 t + 63, with one
// it is a brick of neighbouring gridcells.  Tiles are numbered brick-i fastest, so the waves of a block and the blocks
// of a launch walk neighbouring bricks.  Every row of [0, nrow) lies in exactly one tile.
// (A brick's lanes are checked against sh.nrow alone: every launcher's shape is pick_shape(..., nrow), whose nrow is the
// launch's, or TileShape(), which takes the first branch.)
__device__ __forceinline__ uint64_t tile_row(const TileShape& sh, uint64_t tile_id, int lane, uint64_t nrow,
                                             bool* valid) {
  if (sh.im == 0) {
    const uint64_t row = tile_id * kWave + lane;
    *valid = row < nrow;
    return row;
  }
  uint32_t t = (uint32_t)tile_id;
  const uint32_t bi = t % sh.nbi;
  t /= sh.nbi;
  const uint32_t bj = t % sh.nbj;
  const uint32_t bk = t / sh.nbj;
  const uint32_t l = (uint32_t)lane;
  uint32_t di, dj, dk;
  if (sh.k_fastest) {
    dk = l & ((1u << sh.lk) - 1u);
    di = (l >> sh.lk) & ((1u << sh.li) - 1u);
    dj = l >> (sh.lk + sh.li);
  } else {
    di = l & ((1u << sh.li) - 1u);
    dj = (l >> sh.li) & ((1u << sh.lj) - 1u);
    dk = l >> (sh.li + sh.lj);
  }
  const uint32_t i = (bi << sh.li) + di;
  const uint32_t j = (bj << sh.lj) + dj;
  const uint32_t k = sh.k_first + (bk << sh.lk) + dk;
  const uint64_t m = (uint64_t)i + (uint64_t)sh.im * ((uint64_t)j + (uint64_t)sh.jm * (uint64_t)k);
  *valid = i < sh.im && j < sh.jm && m >= sh.row0 && m - sh.row0 < sh.nrow;
  return m - sh.row0;
}

// ------------------------------------------------------------------ tile fill

// Row-major rows -> the wave's LDS tile as tile[f * 64 + lane] (`tile` is the lane's column; conflict-free: bank =
// lane % 32 whatever the feature).  `missing` values become NaN so the walk has one notion of missing, columns the
// matrix does not have are NaN, a lane without a row gets zeros (it walks and its result is dropped).  Returns whether
// the lane's row has a missing value; raises kFlagInfInput at `flags` (where not null) for +-inf while `missing` is
// finite.  A caller that passes nullptr or drops the result pays for neither.  NONTEMPORAL: the launch reads every row
// once; otherwise the rows are read again (per tree) and left to the caches.
template <bool NONTEMPORAL>
__device__ __forceinline__ bool stage_rows(float* __restrict__ tile, const float* __restrict__ rows, uint64_t row,
                                           bool valid, uint32_t ncol, uint32_t nfeat, float missing, bool missing_is_nan,
                                           uint32_t* flags) {
  bool any_nan = false;
  bool any_inf = false;
  const float qnan = __builtin_nanf("");
  const float* p = rows + row * (uint64_t)ncol;
  uint32_t f = 0;
  if (valid) {
    for (; f + 4 <= ncol; f += 4) {
      f4u v = NONTEMPORAL ? __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p + f))
                          : *reinterpret_cast<const f4u*>(p + f);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float x = v[c];
        any_inf |= is_inf(x);
        if (!missing_is_nan && x == missing) x = qnan;
        any_nan |= (x != x);
        tile[(f + c) * kWave] = x;
      }
    }
    for (; f < ncol; ++f) {
      float x = NONTEMPORAL ? __builtin_nontemporal_load(p + f) : p[f];
      any_inf |= is_inf(x);
      if (!missing_is_nan && x == missing) x = qnan;
      any_nan |= (x != x);
      tile[f * kWave] = x;
    }
    // a booster with more features than the matrix has columns sees them as missing
    for (; f < nfeat; ++f) {
      tile[f * kWave] = qnan;
      any_nan = true;
    }
    if (any_inf && !is_inf(missing) && flags) atomicOr(flags, kFlagInfInput);
  } else {
    for (; f < nfeat; ++f) tile[f * kWave] = 0.0f;
  }
  return any_nan;
}

// ------------------------------------------------------------------ the walk to a leaf index

// The dense leaf index the row reaches in the tree rooted at slot `root` of 16-byte nodes (VisitNode, visits.hpp: value,
// left child or 0 at a leaf, feature | default_left << 31, leaf index).  NaN or `missing` takes the default child, a
// column the matrix lacks is missing, x < cond goes left, +-inf is compared as the float it is.  STAGE: the row's
// values from the LDS tile (stage_rows), else from the row in global memory (x; nullptr for a lane without a row, which
// walks on zeros).
template <bool STAGE>
__device__ __forceinline__ uint32_t walk_to_leaf(__amdgpu_buffer_rsrc_t nodes, uint32_t root, const float* tile,
                                                 const float* x, uint32_t ncol, float missing) {
  const bool missing_is_nan = missing != missing;
  const float qnan = __builtin_nanf("");
  uint4 nd = load_node16(nodes, root);
  while (nd.y != 0u) {
    const uint32_t f = nd.z & 0x7FFFFFFFu;
    float v;
    if (STAGE) {
      v = tile[f * kWave];
    } else {
      v = 0.0f;
      if (x != nullptr) {
        v = qnan;
        if (f < ncol) {
          v = x[f];
          if (!missing_is_nan && v == missing) v = qnan;
        }
      }
    }
    const bool left = (v != v) ? (nd.z >> 31) != 0u : (v < __uint_as_float(nd.x));
    nd = load_node16(nodes, nd.y + (left ? 0u : 1u));
  }
  return nd.w;
}

// counters[key] += 1 for every lane with `counted`, the lanes of the wave that name the same key merged: the first lane
// still to do names its counter and everyone on it is counted with one 64-bit add.  The whole wave calls it together.
__device__ __forceinline__ void add_per_leaf(unsigned long long* counters, uint32_t key, bool counted, int lane) {
  uint64_t todo = __ballot(counted);
  while (todo != 0ull) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
    const uint64_t same = __ballot(counted && key == k);
    if (lane == leader) atomicAdd(&counters[k], (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

// ------------------------------------------------------------------ host

// A kernel that asks for more dynamic LDS than the 64 KiB every kernel may have says so once before its launch.
template <class K>
inline hipError_t raise_lds_limit(K kernel, size_t lds_bytes) {
  if (lds_bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lds_bytes);
}

}  // namespace ohx
#endif  // __HIPCC__
