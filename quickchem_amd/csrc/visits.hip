// gfx950 kernels of the node visit counts (visits.hpp; design in docs/16_visit_counts.md).
//
// One lane owns one row, a wave 64 rows (consecutive ones, or a brick of the caller's grid).  A node is 16 bytes
// (VisitNode) and is fetched with one 128-bit gather per step through a buffer descriptor; a leaf carries its dense
// index inside the tree, and the row adds one to that leaf's counter.  The walk is the margin predict's: NaN or the
// matrix's `missing` takes the default child, a column the matrix lacks is missing, x < cond goes left, +-inf is
// compared as the float it is.
//
// Where the increment goes is what the two kernels differ in.
//   visits_lds_kernel     a block owns ONE tree and a range of tiles, keeps that tree's leaf histogram in LDS as uint32,
//                         counts with LDS atomics and flushes the nonzero counters once, at its end, with 64-bit global
//                         adds on consecutive leaves by consecutive lanes.
//   visits_global_kernel  trees with more leaves than fit: the lanes of a wave that stand on the same leaf are merged
//                         (ballot + popcount) and one 64-bit global add is made per distinct leaf.
// Only integer adds: the two give the same counters, whatever the launch shape.  No float atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "visits.hpp"

namespace ohx {

namespace {

constexpr int kWave = 64;
constexpr int kBlock = (int)kVisitBlock;
constexpr int kWavesPerBlock = kBlock / kWave;

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// One 128-bit load per node that the compiler cannot split, a 32-bit offset, and a hardware range check that turns a
// stray slot into a read of zeros - a leaf of index 0 - instead of a fault (as categorical.hip).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t node_rsrc(const DeviceVisitForest& fr) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<VisitNode*>(fr.nodes), 0, (int)fr.node_bytes, 0x00020000);
}
__device__ __forceinline__ uint4 load_node(__amdgpu_buffer_rsrc_t r, uint32_t slot) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(slot << 4), 0, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// Row of this lane in tile `tile_id` (kernels.hpp TileShape; the walk kernels' own rule): every row of [0, nrow) lies in
// exactly one tile, so every row is counted exactly once per tree.
__device__ __forceinline__ uint64_t tile_row(const TileShape& sh, uint64_t tile_id, int lane, uint64_t nrow, bool* valid) {
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
  *valid = i < sh.im && j < sh.jm && m >= sh.row0 && m - sh.row0 < sh.nrow && m - sh.row0 < nrow;
  return m - sh.row0;
}

// The wave's rows into LDS as tile[feature * 64 + lane] (conflict-free: bank = lane % 32 whatever the feature):
// `missing` -> NaN, columns the matrix does not have -> NaN, a lane without a row -> zeros (it walks and is not counted).
// ONCE: the launch reads every row once (the global kernel), so the loads are nontemporal; the LDS kernel reads the rows
// again for every tree and leaves them to the caches.
template <bool ONCE>
__device__ __forceinline__ void stage_rows(float* tile, const VisitArgs& a, uint32_t num_feature, uint64_t row, bool valid) {
  const bool missing_is_nan = a.missing != a.missing;
  const float qnan = __builtin_nanf("");
  uint32_t f = 0;
  if (valid) {
    const float* p = a.rows + row * (uint64_t)a.ncol;
    for (; f + 4 <= a.ncol; f += 4) {
      const f4u v = ONCE ? __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p + f))
                         : *reinterpret_cast<const f4u*>(p + f);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float x = v[c];
        if (!missing_is_nan && x == a.missing) x = qnan;
        tile[(f + c) * kWave] = x;
      }
    }
    for (; f < a.ncol; ++f) {
      float x = ONCE ? __builtin_nontemporal_load(p + f) : p[f];
      if (!missing_is_nan && x == a.missing) x = qnan;
      tile[f * kWave] = x;
    }
    for (; f < num_feature; ++f) tile[f * kWave] = qnan;
  } else {
    for (; f < num_feature; ++f) tile[f * kWave] = 0.0f;
  }
}

// The dense leaf index the row reaches in the tree rooted at `root`.  STAGE: the row's values from the LDS tile, else
// from the row in global memory (x; nullptr for a lane without a row, which walks on zeros).
template <bool STAGE>
__device__ __forceinline__ uint32_t walk_to_leaf(__amdgpu_buffer_rsrc_t nodes, uint32_t root, const float* tile,
                                                 const float* x, const VisitArgs& a) {
  const bool missing_is_nan = a.missing != a.missing;
  const float qnan = __builtin_nanf("");
  uint4 nd = load_node(nodes, root);
  while (nd.y != 0u) {
    const uint32_t f = nd.z & 0x7FFFFFFFu;
    float v;
    if (STAGE) {
      v = tile[f * kWave];
    } else {
      v = 0.0f;
      if (x != nullptr) {
        v = qnan;
        if (f < a.ncol) {
          v = x[f];
          if (!missing_is_nan && v == a.missing) v = qnan;
        }
      }
    }
    const bool left = (v != v) ? (nd.z >> 31) != 0u : (v < __uint_as_float(nd.x));
    nd = load_node(nodes, nd.y + (left ? 0u : 1u));
  }
  return nd.w;
}

// grid (blocks, trees of this launch); dynamic LDS: the four tiles (STAGE), then a.hist_leaves uint32 counters
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void visits_lds_kernel(DeviceVisitForest fr, VisitArgs a) {
  extern __shared__ float visits_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  float* tile = visits_lds + (size_t)wave * fr.num_feature * kWave + lane;
  uint32_t* hist = reinterpret_cast<uint32_t*>(visits_lds + (STAGE ? (size_t)kWavesPerBlock * fr.num_feature * kWave : 0));
  const uint32_t tree = fr.lds_trees[a.tree_first + blockIdx.y];
  const uint32_t leaf0 = fr.leaf_offset[tree];
  uint32_t nleaf = fr.leaf_offset[tree + 1] - leaf0;
  if (nleaf > a.hist_leaves) nleaf = a.hist_leaves;        // (the plan sized the histogram by its largest tree)
  for (uint32_t i = threadIdx.x; i < nleaf; i += kBlock) hist[i] = 0u;
  __syncthreads();
  const __amdgpu_buffer_rsrc_t nodes = node_rsrc(fr);
  const uint32_t root = fr.roots[tree];
  const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t t64 = a.tile_begin + (uint64_t)blockIdx.x * kWavesPerBlock + wave; t64 < a.tile_end; t64 += nwaves) {
    bool valid;
    const uint64_t row = tile_row(a.shape, t64, lane, a.nrow, &valid);
    if (!__any(valid)) continue;                 // a brick that overhangs the rows altogether
    if (STAGE) stage_rows<false>(tile, a, fr.num_feature, row, valid);
    // (a wave reads only its own tile, each lane only its own column: no barrier)
    const uint32_t leaf = walk_to_leaf<STAGE>(nodes, root, tile, valid ? a.rows + row * (uint64_t)a.ncol : nullptr, a);
    if (valid && leaf < nleaf) atomicAdd(&hist[leaf], 1u);
  }
  __syncthreads();
  // the flush: consecutive leaves by consecutive lanes, 64-bit adds, only where something was counted
  for (uint32_t i = threadIdx.x; i < nleaf; i += kBlock) {
    const uint32_t c = hist[i];
    if (c != 0u) atomicAdd(&a.counts[(uint64_t)leaf0 + i], (unsigned long long)c);
  }
}

// grid (blocks); a wave stages its tile once and walks every tree of the plan's global list
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void visits_global_kernel(DeviceVisitForest fr, VisitArgs a) {
  extern __shared__ float visits_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  float* tile = visits_lds + (size_t)wave * fr.num_feature * kWave + lane;
  const __amdgpu_buffer_rsrc_t nodes = node_rsrc(fr);
  const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t t64 = a.tile_begin + (uint64_t)blockIdx.x * kWavesPerBlock + wave; t64 < a.tile_end; t64 += nwaves) {
    bool valid;
    const uint64_t row = tile_row(a.shape, t64, lane, a.nrow, &valid);
    if (!__any(valid)) continue;
    if (STAGE) stage_rows<true>(tile, a, fr.num_feature, row, valid);
    const float* x = valid ? a.rows + row * (uint64_t)a.ncol : nullptr;
    for (uint32_t q = 0; q < a.tree_count; ++q) {
      const uint32_t tree = fr.global_trees[a.tree_first + q];
      const uint32_t leaf = walk_to_leaf<STAGE>(nodes, fr.roots[tree], tile, x, a);
      const uint32_t key = fr.leaf_offset[tree] + leaf;      // the counter: below 2^32 (emit_visits)
      // lanes on the same leaf merge: the first lane still to do names its counter, everyone on it is counted with one add
      const bool counted = valid && key < fr.total_leaves;
      uint64_t todo = __ballot(counted);
      while (todo != 0ull) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
        const uint64_t same = __ballot(counted && key == k);
        if (lane == leader) atomicAdd(&a.counts[k], (unsigned long long)__popcll(same));
        todo &= ~same;
      }
    }
  }
}

template <class K>
hipError_t raise_lds_limit(K kernel, size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace

int prepare_count_visits(const VisitPlan& plan) {
  hipError_t e = hipSuccess;
  if (!plan.lds_trees.empty()) {
    e = plan.stage ? raise_lds_limit(visits_lds_kernel<true>, plan.lds_bytes_lds)
                   : raise_lds_limit(visits_lds_kernel<false>, plan.lds_bytes_lds);
    if (e != hipSuccess) return e;
  }
  if (!plan.global_trees.empty() && plan.stage) e = raise_lds_limit(visits_global_kernel<true>, plan.lds_bytes_global);
  return e;
}

int launch_count_visits(const DeviceVisitForest& fr, const VisitArgs& args, const VisitPlan& plan, int num_cus,
                        const LaunchTuning& tune, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  VisitArgs a = args;
  if (a.nrow == 0 || fr.num_trees == 0) return hipSuccess;
  if (a.ncol > fr.num_feature || plan.lds_bytes_lds > kVisitCuLdsBytes || plan.lds_bytes_global > kVisitCuLdsBytes ||
      plan.lds_trees.size() + plan.global_trees.size() != fr.num_trees)
    return hipErrorInvalidValue;
  // which rows a wave takes: bricks when the caller named the grid the rows come from, as the walk kernels do
  // (kernels.hpp pick_shape); not when most bricks would hold no row
  a.shape = pick_shape(tune, tune.grid_im, tune.grid_jm, tune.grid_row0, a.nrow);
  if (a.shape.im != 0 && a.shape.live_tiles() * 2 < a.shape.ntiles(a.nrow)) a.shape = TileShape();
  const uint64_t ntiles = a.shape.ntiles(a.nrow);
  a.hist_leaves = plan.hist_leaves;
  hipError_t e = hipSuccess;
  for (uint64_t t0 = 0; t0 < ntiles; t0 += kVisitTilesPerLaunch) {
    a.tile_begin = t0;
    a.tile_end = t0 + kVisitTilesPerLaunch < ntiles ? t0 + kVisitTilesPerLaunch : ntiles;
    const uint64_t span = a.tile_end - a.tile_begin;
    for (size_t q0 = 0; q0 < plan.lds_trees.size(); q0 += kVisitTreesPerLaunch) {
      a.tree_first = (uint32_t)q0;
      a.tree_count = (uint32_t)(plan.lds_trees.size() - q0 < kVisitTreesPerLaunch ? plan.lds_trees.size() - q0 : kVisitTreesPerLaunch);
      const dim3 grid(visit_lds_blocks(span, num_cus), a.tree_count);
      if (plan.stage) hipLaunchKernelGGL(visits_lds_kernel<true>, grid, dim3(kBlock), plan.lds_bytes_lds, stream, fr, a);
      else hipLaunchKernelGGL(visits_lds_kernel<false>, grid, dim3(kBlock), plan.lds_bytes_lds, stream, fr, a);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (!plan.global_trees.empty()) {
      a.tree_first = 0;
      a.tree_count = (uint32_t)plan.global_trees.size();
      const dim3 grid(visit_global_blocks(span, num_cus));
      if (plan.stage) hipLaunchKernelGGL(visits_global_kernel<true>, grid, dim3(kBlock), plan.lds_bytes_global, stream, fr, a);
      else hipLaunchKernelGGL(visits_global_kernel<false>, grid, dim3(kBlock), 0, stream, fr, a);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

}  // namespace ohx
