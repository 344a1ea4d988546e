// Host preparation of per-feature contributions (include/ohxgb.h, OHXBoosterPredictContribs): the tables the
// contribs.hip kernels read, and the float node means both the kernels and the test-support CPU restatement
// (contribs_host.cpp) start from.  Built once per booster and mode, at the first contribs call of that mode.
//
// Node means (xgboost 1.6.0 FillNodeMeanValues, in float, in this order):
//   mean(leaf) = leaf value;  mean(n) = (mean(l) * cover(l) + mean(r) * cover(r)) / cover(n),  cover = sum_hess.
//
// Approximate mode walks ContribNode, the wide node's shape with the node's mean where the wide format keeps the
// original node id: one 16-byte load per step holds the split and both means the step needs.
//
// Exact mode (path-dependent TreeSHAP) walks a path table: every leaf is one path, from the root down, its
// elements the DISTINCT features split on along the way.  An element carries
//   feature | miss << 31   miss = 1 when a missing value takes this path at EVERY occurrence of the feature
//   [lo, hi)               the interval x must lie in to take this path at every occurrence (NaN = unbounded)
//   z                      the product over occurrences of cover(child) / cover(parent)
// so the one fraction of a row is  missing(x) ? miss : !(x < lo) && !(x >= hi).  Element 0 of the algorithm, the bias
// element (z = o = 1), is implicit.  Within a tree the paths are sorted by length class (kPathClassMax) so the kernel
// can run each class through a body unrolled to its maximum length; class_start[t * (kPathClasses + 1) + c] is where
// class c of tree t starts.  Leaves reached without a split (a tree that is one leaf) have no features and are
// not in the table: they only add to the bias column.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "forest.hpp"

namespace ohx {

constexpr int kPathClasses = 7;
constexpr int kPathClassMax[kPathClasses] = {4, 8, 12, 16, 20, 24, 32};
constexpr int kMaxPathLen = 32;         // distinct features on one root-to-leaf path
constexpr uint32_t kMaxContribFeatures = 128;   // two [feature][64] float tiles per wave must fit a block's 64 KiB of LDS

struct ContribNode {   // 16 bytes
  float value;         // split condition, or the leaf value
  uint32_t left;       // absolute index of the left child (right = left + 1), 0 => leaf
  uint32_t feat_dl;    // feature | default_left << 31
  float mean;          // node mean
};

struct PathElem {      // 16 bytes
  uint32_t feat;       // feature | miss << 31
  float lo, hi;        // NaN = unbounded
  float z;
};

struct PathHead {      // 16 bytes
  uint32_t first;      // index of the path's first element
  uint32_t len;        // distinct features, 1 .. kMaxPathLen
  float leaf;
  uint32_t pad;
};

struct PathTable {
  std::vector<PathHead> heads;
  std::vector<PathElem> elems;
  std::vector<uint32_t> class_start;   // [tree][kPathClasses + 1]
  uint64_t sum_sq = 0;                 // sum over paths of (len + 1)^2: the element steps of the recurrences
  uint32_t max_len = 0;
  uint64_t bytes() const {
    return heads.size() * sizeof(PathHead) + elems.size() * sizeof(PathElem) + class_start.size() * sizeof(uint32_t);
  }
};

// Throws OhxError unless every internal node reachable from a root has a finite cover > 0.
void check_contrib_cover(const Forest& f);
// mean of every node of tree t, indexed like the tree's arrays (unreachable nodes: 0)
std::vector<float> node_means(const Tree& t);
// bias column: sum of the root means of trees [t0, t1), in tree order from 0.0f, then + margin_base
float contrib_bias(const Forest& f, const std::vector<std::vector<float>>& means, uint32_t t0, uint32_t t1,
                   float margin_base);
// file-order nodes of every tree, tree after tree; roots[t] = index of tree t's root
std::vector<ContribNode> emit_contrib_nodes(const Forest& f, const std::vector<std::vector<float>>& means,
                                            std::vector<uint32_t>* roots);
// Throws OhxError when a path holds more than kMaxPathLen distinct features.
PathTable build_path_table(const Forest& f);
// the length class of a path of `len` distinct features
int path_class(uint32_t len);

// ---- the launches (contribs.hip) ----

// unwound-sum coefficients per (len, i): {(len+1)/(i+1), (len-i)/(len+1), (len+1)/(len-i), 0}
constexpr int kCoefStride = kMaxPathLen + 1;
std::vector<float> unwind_coefficients();   // [kCoefStride][kCoefStride][4]

struct ContribsArgs {
  const float* rows = nullptr;   // [nrow][ncol], device
  uint64_t nrow = 0;
  uint32_t ncol = 0;
  float missing = 0.0f;
  uint32_t nfeat = 0;            // F: out is [nrow][F + 1]
  uint32_t tree_begin = 0, tree_end = 0;
  float bias = 0.0f;             // column F
  float* out = nullptr;
  uint32_t* flags = nullptr;     // bit 0: +-inf in the rows while `missing` is finite (may be null: not checked)
  // exact mode
  const PathHead* heads = nullptr;
  const PathElem* elems = nullptr;
  const uint32_t* class_start = nullptr;
  const float* coef = nullptr;
  // approximate mode
  const ContribNode* nodes = nullptr;
  const uint32_t* roots = nullptr;
};

constexpr uint64_t kContribsTileRows = 64;            // rows of one tile: one wave, one row per lane
constexpr uint64_t kWaveSlots = 8192;                 // 256 CUs x 32 waves
constexpr uint64_t kPartBudgetBytes = 1ull << 30;     // largest `part` a split may ask for
constexpr uint64_t kDirectTilesPerLaunch = 8192;      // exact mode, direct: tiles per launch (bounds a launch's length)

// How a batch is cut: batches that leave most of the chip's wave slots empty have their trees split over waves,
// every (tile, tree group) writing its trees' contributions to `part` one tree at a time, and a second launch sums
// them in tree order.  Bigger batches: one wave per tile walks every tree.  Either way a row's bits are the same.
struct ContribsPlan {
  bool split = false;
  uint32_t trees_per_group = 0, groups = 0;
  uint64_t part_floats = 0;      // size of `part` the split needs
};
// allow_split = false ("ohx_contribs_split" = off): always direct.  Host logic (contribs.cpp).
ContribsPlan plan_contribs(uint64_t nrow, uint32_t nfeat, uint32_t ntree, bool allow_split);
// Enqueues everything on `stream` (a hipStream_t).  `part` must hold plan.part_floats floats when plan.split.
// Returns a hipError_t.
int launch_contribs(bool approximate, const ContribsArgs& a, const ContribsPlan& plan, float* part, void* stream);

// ---- contributions from the fields (contribs.hip; include/ohxgb.h OHXBoosterPredictContribsFields) ----
//
// The rows are the slab's gridcells m = i + im * (j + jm * k'), gathered in place as the fields predict does (PL / 100,
// 2-D fields broadcast over the levels, `missing` -> NaN, fields past nfield missing), into the row tile of the
// contribs kernels' arithmetic.  Output feature-major: out[f][out_off + m], one array per feature and the bias.
constexpr uint32_t kMaxFieldsFeatures = 32;
struct FieldsContribsArgs {
  const float* field[kMaxFieldsFeatures];      // device; field f is (im,jm) when bit f of is2d_mask is set
  uint32_t is2d_mask = 0;
  uint32_t pl_feature = 0xFFFFFFFFu;           // divided by 100 (0xFFFFFFFF: none)
  uint32_t nfield = 0;
  float missing = 0.0f;
  uint64_t plane = 0;                          // im * jm
  uint64_t nrow = 0;                           // gridcells of the slab
  uint64_t src_off = 0;                        // floats from a 3-D field's pointer to the slab's first level
  uint64_t out_off = 0;                        // the same in the outputs
  float* out[kMaxFieldsFeatures + 1] = {};     // [0, nfeat]: device, nullptr = not stored
  uint32_t* flags = nullptr;                   // bit 0: +-inf in the slab while `missing` is finite (null: not checked)
};
// `a` carries the trees, the bias and the mode's tables (a.rows, a.out unused); plan = plan_contribs(f.nrow, ...).
// Enqueues on `stream`; returns a hipError_t.
int launch_contribs_fields(bool approximate, const ContribsArgs& a, const FieldsContribsArgs& f,
                           const ContribsPlan& plan, float* part, void* stream);

// ---- SHAP interaction values (interactions.hip; include/ohxgb.h OHXBoosterPredictInteractions) ----
//
// Exact mode conditions on one feature i at a time: a wave owns one (64-row tile, feature i, tree group) and walks,
// tree by tree, only the paths that hold i.  The feature-path index lists them: for tree t and feature f,
// paths[start[(t * nfeat + f) * (kPathClasses + 1) + c] ..] are the table's paths of length class c that hold f, in
// table order.  One entry per path element: as many entries as the table has elements (4 bytes each).
struct FeaturePathIndex {
  std::vector<uint32_t> paths;
  std::vector<uint32_t> start;   // [tree][nfeat][kPathClasses + 1]
  uint64_t bytes() const { return (paths.size() + start.size()) * sizeof(uint32_t); }
};
FeaturePathIndex build_feature_path_index(const PathTable& pt, uint32_t ntree, uint32_t nfeat);

struct InteractionsArgs {
  const float* rows = nullptr;   // [nrow][ncol], device
  uint64_t nrow = 0;
  uint32_t ncol = 0;
  float missing = 0.0f;
  uint32_t nfeat = 0;            // F: out is [nrow][F + 1][F + 1]
  uint32_t tree_begin = 0, tree_end = 0;
  const float* phi = nullptr;    // [nrow][F + 1]: the same rows' contributions over the same trees, same mode
  float* out = nullptr;
  // exact mode
  const PathHead* heads = nullptr;
  const PathElem* elems = nullptr;
  const uint32_t* fpaths = nullptr;   // FeaturePathIndex
  const uint32_t* fstart = nullptr;
  const float* coef = nullptr;
};

// Exact mode's launch shape.  A direct wave is one (tile, feature); a batch whose direct waves leave most of the
// chip's wave slots empty has its trees split over waves, every (tile, feature, tree group) wave storing each tree's
// matrix row in `part` (tiles x nfeat x ntree x nfeat x 64 floats, at most kPartBudgetBytes), summed in tree order by
// a second launch.  Direct launches hold at most kDirectTilesPerLaunch waves.  Host logic (contribs.cpp).
ContribsPlan plan_interactions(uint64_t nrow, uint32_t nfeat, uint32_t ntree, bool allow_split);
inline uint64_t interactions_tiles_per_launch(uint32_t nfeat) {
  return nfeat == 0 || nfeat >= kDirectTilesPerLaunch ? 1 : kDirectTilesPerLaunch / nfeat;
}
// Enqueues on `stream`, after the launch that filled a.phi: exact mode's off-diagonals (plan, `part`), then the
// diagonal and the bias row and column.  Approximate mode: the diagonal only, off-diagonals 0.  Returns a hipError_t.
int launch_interactions(bool approximate, const InteractionsArgs& a, const ContribsPlan& plan, float* part,
                        void* stream);

}  // namespace ohx
