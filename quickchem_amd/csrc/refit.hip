// gfx950 kernels of the leaf refit (refit.hpp; design in docs/17_leaf_refit.md).
//
// One lane owns one row, a wave 64 consecutive rows.  Three kernels, enqueued back to back:
//   refit_leaf_ids_kernel    once: a wave stages its rows, walks ALL trees (the visit counts' walk over the 16-byte
//                            VisitNode; no leaf value is read), stores each tree's dense leaf id at ids[t][row] and adds
//                            the rows per leaf into H, the lanes of a wave on one leaf merged into one 64-bit add.
//   refit_accumulate_kernel  once per tree t: pred += the refit leaf of tree t-1, g = pred - label, q = rint(g * 2^24);
//                            the q of the lanes of a wave that stand on one leaf are summed across the wave and added
//                            into G[leaf] with one 64-bit integer add (adding lane by lane gave the same integers and
//                            measured 1.4 times slower per tree: docs/17_leaf_refit.md 17.4).
//   refit_solve_kernel       once per tree t: a thread per leaf, refit_solve_leaf (refit.hpp).
// Only integer adds: no float atomics, and the same sums whatever the order of the rows or the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "refit.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kRefitBlock;
constexpr int kWavesPerBlock = kBlock / kWave;

// grid (blocks); dynamic LDS: the four tiles (STAGE)
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void refit_leaf_ids_kernel(RefitArgs a) {
  extern __shared__ float refit_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const DeviceLeafWalk& w = a.walk;
  float* tile = refit_lds + (size_t)wave * w.num_feature * kWave + lane;
  const bool missing_is_nan = a.missing != a.missing;
  const __amdgpu_buffer_rsrc_t nodes = make_rsrc(w.nodes, w.node_bytes);
  const uint64_t ntiles = (a.nrow + kWave - 1) / kWave;
  const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t t64 = (uint64_t)blockIdx.x * kWavesPerBlock + wave; t64 < ntiles; t64 += nwaves) {
    const uint64_t row = t64 * kWave + lane;
    const bool valid = row < a.nrow;
    // the launch reads every row once: nontemporal loads
    if (STAGE) (void)stage_rows<true>(tile, a.rows, row, valid, a.ncol, w.num_feature, a.missing, missing_is_nan, nullptr);
    // (a wave reads only its own tile, each lane only its own column: no barrier)
    const float* x = valid ? a.rows + row * (uint64_t)a.ncol : nullptr;
    for (uint32_t tree = 0; tree < w.num_trees; ++tree) {
      const uint32_t leaf = walk_to_leaf<STAGE>(nodes, w.roots[tree], tile, x, a.ncol, a.missing);
      const uint32_t key = w.leaf_offset[tree] + leaf;
      // tree-major planes: the wave's 64 ids are 256 contiguous bytes
      if (valid) __builtin_nontemporal_store(leaf, a.ids + (uint64_t)tree * a.nrow + row);
      // the rows per leaf
      add_per_leaf(a.H, key, valid && key < w.total_leaves, lane);
    }
  }
}

// grid (blocks); tree = the tree whose sums are made.  pred is written here for the first time at tree 0.
__global__ __launch_bounds__(kBlock) void refit_accumulate_kernel(RefitArgs a, uint32_t tree) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t leaf0 = a.walk.leaf_offset[tree];
  const uint32_t nleaf = a.walk.leaf_offset[tree + 1] - leaf0;
  uint32_t prev0 = 0, nprev = 0;
  if (tree != 0) {
    prev0 = a.walk.leaf_offset[tree - 1];
    nprev = leaf0 - prev0;
  }
  const uint32_t* ids = a.ids + (uint64_t)tree * a.nrow;
  const uint32_t* ids_prev = tree != 0 ? ids - a.nrow : nullptr;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  // whole waves run the loop together (the ballots below): the bound is rounded up to the wave
  const uint64_t bound = (a.nrow + kWave - 1) / kWave * kWave;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < bound; row += stride) {
    const bool valid = row < a.nrow;
    uint32_t flags = 0;
    bool add = false;
    uint32_t key = 0;
    long long q = 0;
    if (valid) {
      float p = a.base;
      if (tree != 0) {
        p = a.pred[row];
        const uint32_t lp = __builtin_nontemporal_load(ids_prev + row);
        if (lp < nprev) p += a.leaf[prev0 + lp];
        else flags |= kRefitFlagLeafId;
      }
      a.pred[row] = p;
      const float g = p - __builtin_nontemporal_load(a.labels + row);
      const uint32_t leaf = ids[row];
      if (leaf >= nleaf) flags |= kRefitFlagLeafId;
      // (a NaN fails the comparison)
      if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) flags |= kRefitFlagLabel;
      if (flags == 0) {
        q = (long long)__builtin_rintf(g * kRefitGradScale);
        key = leaf0 + leaf;
        add = true;
      }
    }
    if (flags != 0) atomicOr(a.error, flags);
    // lanes on the same leaf merge: the first lane still to do names its leaf, the q of everyone on it are summed
    // across the wave and added once
    uint64_t todo = __ballot(add);
    while (todo != 0ull) {
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
      const bool mine = add && key == k;
      const uint64_t same = __ballot(mine);
      long long s = mine ? q : 0ll;
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) s += __shfl_xor(s, d, kWave);
      if (lane == leader) atomicAdd(&a.G[k], (unsigned long long)s);
      todo &= ~same;
    }
  }
}

// grid (blocks over the tree's leaves)
__global__ __launch_bounds__(kBlock) void refit_solve_kernel(RefitArgs a, uint32_t tree) {
  const uint32_t leaf0 = a.walk.leaf_offset[tree];
  const uint32_t nleaf = a.walk.leaf_offset[tree + 1] - leaf0;
  const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
  if (l >= nleaf) return;
  const uint32_t k = leaf0 + l;
  const unsigned long long H = a.H[k];
  if (H == 0ull) {
    if (a.unvisited != 0) a.leaf[k] = a.weight[k] = 0.0f;
    return;
  }
  float leaf, weight;
  refit_solve_leaf((int64_t)a.G[k], (uint64_t)H, a.eta, a.lambda, &leaf, &weight);
  a.leaf[k] = leaf;
  a.weight[k] = weight;
}

}  // namespace

int prepare_refit(const RefitPlan& plan) {
  return plan.stage ? raise_lds_limit(refit_leaf_ids_kernel<true>, plan.lds_bytes) : hipSuccess;
}

int launch_refit(const RefitArgs& a, const RefitPlan& plan, const uint32_t* leaf_offset, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (a.nrow == 0 || a.walk.num_trees == 0) return hipSuccess;
  if (a.nrow > kRefitMaxRows || a.ncol > a.walk.num_feature || plan.lds_bytes > kVisitStageMaxBytes || plan.ids_blocks == 0 ||
      plan.accum_blocks == 0 || plan.stage != visit_stages(a.walk.num_feature))
    return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (plan.stage) hipLaunchKernelGGL(refit_leaf_ids_kernel<true>, dim3(plan.ids_blocks), dim3(kBlock), plan.lds_bytes, stream, a);
  else hipLaunchKernelGGL(refit_leaf_ids_kernel<false>, dim3(plan.ids_blocks), dim3(kBlock), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (uint32_t t = 0; t < a.walk.num_trees; ++t) {
    hipLaunchKernelGGL(refit_accumulate_kernel, dim3(plan.accum_blocks), dim3(kBlock), 0, stream, a, t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t leaves = leaf_offset[t + 1] - leaf_offset[t];
    if (leaves == 0) continue;
    hipLaunchKernelGGL(refit_solve_kernel, dim3(refit_solve_blocks(leaves)), dim3(kBlock), 0, stream, a, t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ohx
