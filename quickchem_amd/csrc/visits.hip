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
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kVisitBlock;
constexpr int kWavesPerBlock = kBlock / kWave;

// grid (blocks, trees of this launch); dynamic LDS: the four tiles (STAGE), then a.hist_leaves uint32 counters
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void visits_lds_kernel(DeviceVisitForest fr, VisitArgs a) {
  extern __shared__ float visits_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const DeviceLeafWalk& w = fr.walk;
  float* tile = visits_lds + (size_t)wave * w.num_feature * kWave + lane;
  uint32_t* hist = reinterpret_cast<uint32_t*>(visits_lds + (STAGE ? (size_t)kWavesPerBlock * w.num_feature * kWave : 0));
  const uint32_t tree = fr.lds_trees[a.tree_first + blockIdx.y];
  const uint32_t leaf0 = w.leaf_offset[tree];
  uint32_t nleaf = w.leaf_offset[tree + 1] - leaf0;
  if (nleaf > a.hist_leaves) nleaf = a.hist_leaves;        // (the plan sized the histogram by its largest tree)
  for (uint32_t i = threadIdx.x; i < nleaf; i += kBlock) hist[i] = 0u;
  __syncthreads();
  const bool missing_is_nan = a.missing != a.missing;
  const __amdgpu_buffer_rsrc_t nodes = make_rsrc(w.nodes, w.node_bytes);
  const uint32_t root = w.roots[tree];
  const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t t64 = a.tile_begin + (uint64_t)blockIdx.x * kWavesPerBlock + wave; t64 < a.tile_end; t64 += nwaves) {
    bool valid;
    const uint64_t row = tile_row(a.shape, t64, lane, a.nrow, &valid);
    if (!__any(valid)) continue;                 // a brick that overhangs the rows altogether
    // the block reads its rows again for every tree: left to the caches
    if (STAGE) (void)stage_rows<false>(tile, a.rows, row, valid, a.ncol, w.num_feature, a.missing, missing_is_nan, nullptr);
    // (a wave reads only its own tile, each lane only its own column: no barrier)
    const uint32_t leaf = walk_to_leaf<STAGE>(nodes, root, tile, valid ? a.rows + row * (uint64_t)a.ncol : nullptr, a.ncol,
                                              a.missing);
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
  const DeviceLeafWalk& w = fr.walk;
  float* tile = visits_lds + (size_t)wave * w.num_feature * kWave + lane;
  const bool missing_is_nan = a.missing != a.missing;
  const __amdgpu_buffer_rsrc_t nodes = make_rsrc(w.nodes, w.node_bytes);
  const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t t64 = a.tile_begin + (uint64_t)blockIdx.x * kWavesPerBlock + wave; t64 < a.tile_end; t64 += nwaves) {
    bool valid;
    const uint64_t row = tile_row(a.shape, t64, lane, a.nrow, &valid);
    if (!__any(valid)) continue;
    // the launch reads every row once: nontemporal loads
    if (STAGE) (void)stage_rows<true>(tile, a.rows, row, valid, a.ncol, w.num_feature, a.missing, missing_is_nan, nullptr);
    const float* x = valid ? a.rows + row * (uint64_t)a.ncol : nullptr;
    for (uint32_t q = 0; q < a.tree_count; ++q) {
      const uint32_t tree = fr.global_trees[a.tree_first + q];
      const uint32_t leaf = walk_to_leaf<STAGE>(nodes, w.roots[tree], tile, x, a.ncol, a.missing);
      const uint32_t key = w.leaf_offset[tree] + leaf;      // the counter: below 2^32 (emit_visits)
      add_per_leaf(a.counts, key, valid && key < w.total_leaves, lane);
    }
  }
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
  if (a.nrow == 0 || fr.walk.num_trees == 0) return hipSuccess;
  if (a.ncol > fr.walk.num_feature || plan.lds_bytes_lds > kVisitCuLdsBytes || plan.lds_bytes_global > kVisitCuLdsBytes ||
      plan.lds_trees.size() + plan.global_trees.size() != fr.walk.num_trees)
    return hipErrorInvalidValue;
  a.shape = pick_shape_dense(tune, a.nrow);
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
