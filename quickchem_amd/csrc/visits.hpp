// Node visit counts (include/ohxgb.h OHXBoosterCountVisits; design in docs/16_visit_counts.md): how many rows of the
// caller's data pass every node of every tree, and the covers (sum_hess) refreshed from those counts.
//
// The device counts LEAVES: a row walks every tree exactly as a margin predict does and adds one to the counter of the
// leaf it ends on.  The host sums the leaf counters up each tree, so a split's count is the sum of its children's by
// construction.  Everything is an integer: no float atomics, and the same numbers whatever the launch shape.
//
// The walk (walk_device.hpp walk_to_leaf) reads a 16-byte node of its own, VisitNode: the wide node's shape and placement (flatten.hpp WideNode,
// place_forest) with the tree's DENSE LEAF INDEX where the wide format keeps the file's node id.  Leaves are numbered
// 0 .. leaf_count[t] - 1 per tree in file node order; leaf_offset[t] is where tree t's counters start in the one
// uint64 array of the booster.
#pragma once
#include <cstdint>
#include <vector>

#include "flatten.hpp"
#include "forest.hpp"
#ifdef __HIPCC__
#include "kernels.hpp"   // TileShape, LaunchTuning: the launch section below, for what hipcc compiles
#endif

namespace ohx {

struct VisitNode {   // 16 bytes
  float value;       // split condition (unused at a leaf)
  uint32_t left;     // absolute slot of the left child (right = left + 1), 0 => leaf
  uint32_t feat_dl;  // feature | default_left << 31
  uint32_t leaf;     // leaves: the dense leaf index inside the tree
};
static_assert(sizeof(VisitNode) == 16, "one 128-bit load per node");

struct VisitForest {
  std::vector<VisitNode> nodes;         // [num_slots]
  std::vector<uint32_t> roots;          // slot of each tree's root
  std::vector<uint32_t> leaf_offset;    // T + 1: tree t's counters are [leaf_offset[t], leaf_offset[t + 1])
  std::vector<uint32_t> leaf_node;      // [leaf_offset[T]]: the file node of every leaf counter
  std::vector<uint64_t> tree_offsets;   // T + 1: tree t's nodes are [tree_offsets[t], tree_offsets[t + 1]) of the node counts
  uint32_t leaves(uint32_t t) const { return leaf_offset[t + 1] - leaf_offset[t]; }
};
// Throws OhxError when the nodes would not fit a buffer descriptor (4 GiB).
VisitForest emit_visits(const Forest& f, const Placement& p);

// Leaf counters -> node counts in file numbering: a leaf its counter, a split the sum of its children, unreachable and
// deleted slots 0.  node_counts holds tree_offsets[T] entries.
void visit_node_sums(const Forest& f, const VisitForest& vf, const uint64_t* leaf_counts, uint64_t* node_counts);

// sum_hess := (float)count + prior_weight * sum_hess_old for every reachable node, in float32, the product rounded and
// then the sum.  Returns the new covers per tree (unreachable nodes keep their old value) and changes nothing;
// throws OhxError - naming the first tree and node - when a SPLIT's new cover would not be finite and > 0.
std::vector<std::vector<float>> refreshed_covers(const Forest& f, const VisitForest& vf, const uint64_t* node_counts,
                                                 float prior_weight);

// ---- the launches (visits.hip) ----

constexpr size_t kVisitCuLdsBytes = 160 * 1024;
constexpr uint32_t kVisitBlock = 256;               // four waves: four 64-row tiles in flight per block
// rows are staged in LDS as [feature][lane] where the four tiles of a block leave room for a histogram beside them
constexpr size_t kVisitStageMaxBytes = 128 * 1024;
// blocks of one launch: the LDS kernel per tree (x) at most one per CU, the global kernel at most four per CU; a block
// strides over the tiles, so one trip of a kernel's loop is (its blocks) x 4 tiles x 64 rows
constexpr uint32_t kVisitLdsBlocksPerCu = 1, kVisitGlobalBlocksPerCu = 4;
// trees of one LDS launch (gridDim.y), and tiles of one launch: a block's uint32 histogram cannot overflow below 2^32 rows
constexpr uint32_t kVisitTreesPerLaunch = 65535;
constexpr uint64_t kVisitTilesPerLaunch = 1ull << 25;

inline size_t visit_tile_bytes(uint32_t num_feature) { return (size_t)(kVisitBlock / 64) * num_feature * 64 * sizeof(float); }
inline bool visit_stages(uint32_t num_feature) { return num_feature != 0 && visit_tile_bytes(num_feature) <= kVisitStageMaxBytes; }
// leaves a block's LDS histogram can hold beside the staged tiles
inline uint32_t visit_lds_capacity(uint32_t num_feature) {
  return (uint32_t)((kVisitCuLdsBytes - (visit_stages(num_feature) ? visit_tile_bytes(num_feature) : 0)) / sizeof(uint32_t));
}

// Which trees keep their leaf histogram in LDS (a block owns one tree and a range of tiles, counts with LDS atomics and
// flushes its nonzero counters once with contiguous 64-bit global adds) and which are counted the plain way (the lanes
// of a wave that stand on the same leaf merged, one 64-bit global add per distinct leaf).  lds_leaves: the knob
// "ohx_visits_lds_leaves" (0 = the capacity); force_global: "ohx_visits_kernel" = global or auto - the global way
// measured 2.3 times faster than the LDS way on the C360 L72 batch (docs/16_visit_counts.md 16.4), so LDS is by request.
struct VisitPlan {
  std::vector<uint32_t> lds_trees, global_trees;
  uint32_t hist_leaves = 0;     // the largest leaf count among lds_trees: words of a block's histogram
  bool stage = false;
  size_t lds_bytes_lds = 0, lds_bytes_global = 0;   // dynamic LDS of the two kernels
};
VisitPlan plan_visits(const VisitForest& vf, uint32_t num_feature, uint32_t lds_leaves, bool force_global);
// blocks (x) of the two kernels for `ntiles` tiles of one launch
inline uint32_t visit_lds_blocks(uint64_t ntiles, int num_cus) {
  const uint64_t want = (ntiles + kVisitBlock / 64 - 1) / (kVisitBlock / 64), cap = (uint64_t)num_cus * kVisitLdsBlocksPerCu;
  return (uint32_t)(want < cap ? want : cap);
}
inline uint32_t visit_global_blocks(uint64_t ntiles, int num_cus) {
  const uint64_t want = (ntiles + kVisitBlock / 64 - 1) / (kVisitBlock / 64), cap = (uint64_t)num_cus * kVisitGlobalBlocksPerCu;
  return (uint32_t)(want < cap ? want : cap);
}

#ifdef __HIPCC__
// The VisitForest on the device: what a walk to dense leaf indices reads (walk_device.hpp walk_to_leaf).  One per
// booster, shared by the visit counts and the leaf refit; no kernel writes to it.
struct DeviceLeafWalk {
  const VisitNode* nodes = nullptr;
  uint32_t node_bytes = 0;                  // of `nodes` (< 4 GiB: read through a buffer descriptor)
  const uint32_t* roots = nullptr;
  const uint32_t* leaf_offset = nullptr;    // T + 1
  uint32_t num_trees = 0, num_feature = 0;
  uint32_t total_leaves = 0;                // leaf_offset[num_trees]: the counters
};

struct DeviceVisitForest {
  DeviceLeafWalk walk;
  const uint32_t* lds_trees = nullptr;      // the plan's lists
  const uint32_t* global_trees = nullptr;
};

struct VisitArgs {
  const float* rows = nullptr;   // [nrow][ncol], device
  uint64_t nrow = 0;
  uint32_t ncol = 0;
  float missing = 0.0f;
  unsigned long long* counts = nullptr;   // [leaf_offset[T]] leaf counters, added to
  uint64_t tile_begin = 0, tile_end = 0;  // set by the launcher
  uint32_t tree_first = 0, tree_count = 0;   // positions in the plan's list, set by the launcher
  uint32_t hist_leaves = 0;
  TileShape shape;
};
// Once per plan and device, before the first launch with it: lifts the kernels' dynamic LDS limit to what the plan
// asks for.  Returns a hipError_t.
int prepare_count_visits(const VisitPlan& plan);
// Enqueues on `stream` (a hipStream_t): the LDS kernel over plan.lds_trees, then the global kernel over
// plan.global_trees.  Returns a hipError_t.
int launch_count_visits(const DeviceVisitForest& fr, const VisitArgs& a, const VisitPlan& plan, int num_cus,
                        const LaunchTuning& tune, void* stream);
#endif  // __HIPCC__

}  // namespace ohx
