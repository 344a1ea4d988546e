// Test support (libohx_synth.so): the host pieces of the leaf refit (refit.hpp) without a GPU - the solve arithmetic on
// injected sums, the write-back through the leaf maps, and the launch plan.  The product library runs the same
// functions of refit.cpp behind OHXBoosterRefitLeaves.
#include <cstring>
#include <string>
#include <vector>

#include "refit.hpp"

namespace ohx {
void synth_set_error(const std::string& m);   // synth_host.cpp
}

using namespace ohx;

// value / base_weight: n old leaves in, the refit ones out; *refit = the leaves with H > 0
extern "C" __attribute__((visibility("default"))) int ohx_refit_solve(const int64_t* G, const uint64_t* H, uint64_t n,
                                                                     float eta, float lambda, int unvisited, float* value,
                                                                     float* base_weight, uint64_t* refit) {
  try {
    *refit = refit_solve(G, H, n, eta, lambda, unvisited, value, base_weight);
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// The forest's value and base_weight arrays, tree after tree in file numbering (tree_offsets of ohx_visits_layout),
// after leaf tables `value` / `base_weight` (nleaf entries, the dense numbering of ohx_visits_layout) are written back.
// old_value / old_base_weight (may be NULL) receive the leaf tables the forest held before.
extern "C" __attribute__((visibility("default"))) int ohx_refit_write_back(const void* model, uint64_t len, const float* value,
                                                                          const float* base_weight, uint64_t nleaf,
                                                                          float* old_value, float* old_base_weight,
                                                                          float* node_value, float* node_base_weight,
                                                                          uint64_t nnode) {
  try {
    Forest f = load_model_buffer(model, (size_t)len);
    f.validate();
    const VisitForest vf = emit_visits(f, place_forest(f, LayoutParams()));
    if (nleaf != vf.leaf_node.size() || nnode != vf.tree_offsets.back())
      throw OhxError("ohx_refit_write_back: the booster has " + std::to_string(vf.leaf_node.size()) + " leaves and " +
                     std::to_string(vf.tree_offsets.back()) + " nodes");
    std::vector<float> ov(nleaf + 1), ob(nleaf + 1);
    refit_gather_leaves(f, vf, ov.data(), ob.data());
    if (old_value != nullptr && nleaf) memcpy(old_value, ov.data(), nleaf * sizeof(float));
    if (old_base_weight != nullptr && nleaf) memcpy(old_base_weight, ob.data(), nleaf * sizeof(float));
    refit_write_back(f, vf, value, base_weight);
    for (size_t t = 0; t < f.trees.size(); ++t) {
      if (f.trees[t].size() == 0) continue;
      memcpy(node_value + vf.tree_offsets[t], f.trees[t].value.data(), f.trees[t].size() * sizeof(float));
      memcpy(node_base_weight + vf.tree_offsets[t], f.trees[t].base_weight.data(), f.trees[t].size() * sizeof(float));
    }
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// info: [0] rows staged in LDS, [1] dynamic LDS bytes of the leaf-id walk, [2] / [3] blocks of the leaf-id walk / the
// accumulate pass, [4] bytes of the leaf-id planes, [5] rows a block takes per trip (both kernels), [6] / [7] the two
// kernels' block caps per CU
extern "C" __attribute__((visibility("default"))) int ohx_refit_plan(uint64_t nrow, uint32_t num_feature, uint64_t ntree,
                                                                    int num_cus, uint64_t info[8]) {
  try {
    const RefitPlan p = plan_refit(nrow, num_feature, ntree, num_cus);
    info[0] = p.stage ? 1 : 0;
    info[1] = p.lds_bytes;
    info[2] = p.ids_blocks;
    info[3] = p.accum_blocks;
    info[4] = p.ids_bytes;
    info[5] = kRefitBlock;
    info[6] = kRefitIdsBlocksPerCu;
    info[7] = kRefitAccumBlocksPerCu;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}
