// Leaf refit (include/ohxgb.h OHXBoosterRefitLeaves; design in docs/17_leaf_refit.md): every tree keeps its structure
// and every leaf value is estimated again from the caller's rows and labels - xgboost's process_type = update,
// updater = refresh, refresh_leaf = 1 for reg:squarederror (gradient pred - label, hessian 1).
//
// Tree t's gradient depends on the refit leaves of trees 0 .. t-1, so the device makes one pass over the rows per tree.
// What does not depend on leaf values - which leaf a row reaches - is computed once, for all trees, by one walk that
// stores dense leaf ids (visits.hpp VisitForest numbering) tree-major.  The walk reads the booster's one DeviceLeafWalk,
// which the visit counts read too, with the routines of walk_device.hpp.  The per-leaf sums are integers: the gradient in
// fixed point (2^-24) as int64, the hessian a count of rows.  No float atomics, and the same sums whatever the order of
// the rows or the launch shape.
#pragma once
#include <cmath>
#include <cstdint>

#include "visits.hpp"

#ifdef __HIPCC__
#define OHX_REFIT_HD __host__ __device__
#else
#define OHX_REFIT_HD
#endif

namespace ohx {

// g = pred - label must be finite with |g| < kRefitMaxAbsGrad: |q| = |rint(g * 2^24)| < 2^32, and at most 2^31 rows,
// is what keeps a leaf's sum inside an int64
constexpr float kRefitGradScale = 16777216.0f;   // 2^24: the product g * 2^24 is exact in float32
constexpr float kRefitMaxAbsGrad = 256.0f;
constexpr uint64_t kRefitMaxRows = 1ull << 31;
constexpr uint32_t kRefitFlagLabel = 1u;         // the error word: a gradient out of range (a label, or a leaf it made)
constexpr uint32_t kRefitFlagLeafId = 2u;        // a stored leaf id outside its tree (never, from a sound node buffer)

// One leaf from its sums.  CalcWeight of xgboost 1.6.0 with reg_alpha = 0, max_delta_step = 0, min_child_weight <= 1:
// w = -G / (H + lambda), in double and rounded to float once; the leaf is w * eta, one float32 multiply (the
// translation units are built with -ffp-contract=off).  The same function on the host and in refit_solve_kernel.
OHX_REFIT_HD inline void refit_solve_leaf(int64_t G, uint64_t H, float eta, float lambda, float* leaf, float* weight) {
  const float w = (float)(-((double)G * (1.0 / 16777216.0)) / ((double)H + (double)lambda));
  *weight = w;
  *leaf = w * eta;
}

// n leaves: value / base_weight hold the old ones on entry and the new ones on return.  A leaf no row reached (H == 0)
// keeps both (unvisited == 0) or gets +0.0f in both (unvisited != 0).  Returns the leaves with H > 0.
uint64_t refit_solve(const int64_t* G, const uint64_t* H, uint64_t n, float eta, float lambda, int unvisited, float* value,
                     float* base_weight);

// Leaf tables in the VisitForest's dense numbering <-> the forest's node arrays (vf.leaf_node).  Only value and
// base_weight of leaves are read or written.
void refit_gather_leaves(const Forest& f, const VisitForest& vf, float* value, float* base_weight);
void refit_write_back(Forest& f, const VisitForest& vf, const float* value, const float* base_weight);

// ---- the launches (refit.hip) ----

constexpr uint32_t kRefitBlock = 256;   // four waves, one row per lane
// a block strides over its items: the leaf-id walk over tiles of 64 rows (at most four blocks per CU, as
// visits_global_kernel), the accumulate pass over rows (eight per CU: it streams and holds no LDS)
constexpr uint32_t kRefitIdsBlocksPerCu = 4, kRefitAccumBlocksPerCu = 8;

struct RefitPlan {
  bool stage = false;        // the walk stages its rows in LDS (visit_stages)
  size_t lds_bytes = 0;      // dynamic LDS of refit_leaf_ids_kernel
  uint32_t ids_blocks = 0;   // blocks of refit_leaf_ids_kernel: one trip of its loop is ids_blocks x 256 rows
  uint32_t accum_blocks = 0; // blocks of refit_accumulate_kernel: one trip is accum_blocks x 256 rows
  uint64_t ids_bytes = 0;    // the leaf-id planes: ntree x nrow x 4
};
RefitPlan plan_refit(uint64_t nrow, uint32_t num_feature, uint64_t ntree, int num_cus);
inline uint32_t refit_solve_blocks(uint32_t leaves) { return (leaves + kRefitBlock - 1) / kRefitBlock; }

#ifdef __HIPCC__
struct RefitArgs {
  DeviceLeafWalk walk;                     // the VisitForest on the device (visits.hpp)
  // the rows
  const float* rows = nullptr;             // [nrow][ncol]
  uint64_t nrow = 0;
  uint32_t ncol = 0;
  float missing = 0.0f;
  const float* labels = nullptr;           // [nrow]
  // the refit's own buffers
  uint32_t* ids = nullptr;                 // [T][nrow] dense leaf ids
  float* pred = nullptr;                   // [nrow] the margin before the tree at hand
  unsigned long long* G = nullptr;         // [total_leaves] int64 sums of q, added to as two's complement
  unsigned long long* H = nullptr;         // [total_leaves] rows
  float* leaf = nullptr;                   // [total_leaves] old values on entry, new ones as the trees are solved
  float* weight = nullptr;                 // [total_leaves] base_weight, likewise
  uint32_t* error = nullptr;               // one word of kRefitFlag*
  float base = 0.0f, eta = 0.0f, lambda = 0.0f;
  int unvisited = 0;
};
// Once per device before the first launch: the walk's dynamic LDS limit.  Returns a hipError_t.
int prepare_refit(const RefitPlan& plan);
// Enqueues on `stream` (a hipStream_t) the leaf-id walk and then, tree after tree, the accumulate pass and the solve:
// 2T + 1 launches, nothing in between.  G, H and the error word must be zero; leaf_offset is the host's copy of
// a.walk.leaf_offset (a solve launch is sized by its tree's leaves).  Returns a hipError_t.
int launch_refit(const RefitArgs& a, const RefitPlan& plan, const uint32_t* leaf_offset, void* stream);
#endif  // __HIPCC__

}  // namespace ohx
