// Launchers of the gfx950 kernels that predict boosters with categorical splits (definitions in categorical.hip;
// semantics in include/ohxgb.h and docs/14_categorical.md).  Such a booster is walked from a node format of its own
// (flatten.hpp CatNode) and by these kernels only: nothing here is reached by a booster without a categorical split.
// Which rows a wave takes, the fill of its LDS tile and the node load are the walk kernels' (walk_device.hpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "flatten.hpp"
#include "kernels.hpp"

namespace ohx {

struct DeviceCatForest {
  const CatNode* nodes = nullptr;     // [num_slots]
  uint32_t node_bytes = 0;            // of `nodes` (< 4 GiB: read through a buffer descriptor)
  const uint32_t* words = nullptr;    // the sets that do not fit a node (may be null: every set is inline)
  const int32_t* orig_id = nullptr;   // [num_slots] node id in the model file (pred_leaf)
  const uint32_t* roots = nullptr;    // [num_trees] slot of each tree's root
  uint32_t num_trees = 0;
  uint32_t num_feature = 0;
  float base_score = 0.0f;
};

struct CatPredictArgs {
  const float* rows = nullptr;        // [nrow][ncol] row-major
  uint64_t nrow = 0;
  uint32_t ncol = 0;
  float missing = 0.0f;
  uint32_t tree_begin = 0, tree_end = 0;
  float* out = nullptr;               // [nrow] margins, or [nrow][tree_end - tree_begin] leaf ids when pred_leaf
  bool pred_leaf = false;
  uint32_t* flags = nullptr;          // flags[0] |= kFlagInfInput (kernels.hpp) for +-inf in a row while `missing` is finite
  // tile kernel, filled by the launcher: which 64 rows a wave takes (kernels.hpp TileShape: bricks of neighbouring
  // gridcells when the caller named the grid the rows come from, else 64 consecutive rows) and how many tiles there are
  TileShape shape;
  uint64_t ntiles = 0;
};

// Which kernel a predict takes: the tile kernel (a wave's 64 rows staged in LDS, feature-major) for margins when a
// block's four tiles fit a CU's LDS, the direct kernel (no LDS, any feature count) otherwise and for leaf ids.
// force_direct: test and measurement hook ("ohx_cat_kernel" = direct); both kernels give the same bits.
bool cat_uses_tile(uint32_t num_feature, bool pred_leaf, bool force_direct);
const char* cat_kernel_symbol(uint32_t num_feature, bool pred_leaf, bool force_direct);
// tune: the grid of the rows (grid_im, grid_jm, grid_row0) and the brick knobs; nothing else of it is read
hipError_t launch_predict_cat(const DeviceCatForest& forest, const CatPredictArgs& a, int num_cus, bool force_direct,
                              hipStream_t stream, const LaunchTuning& tune = LaunchTuning());

}  // namespace ohx
