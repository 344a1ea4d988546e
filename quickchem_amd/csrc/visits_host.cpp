// Test support (libohx_synth.so): the host pieces of the node visit counts (visits.hpp) without a GPU - the leaf maps,
// leaf counters to node sums, the refresh arithmetic on injected counts, and the launch plan.  The product library
// runs the same functions of visits.cpp behind OHXBoosterGetVisitCounts and OHXBoosterRefreshCover.
#include <cstring>
#include <string>

#include "visits.hpp"

namespace ohx {
void synth_set_error(const std::string& m);   // synth_host.cpp
}

using namespace ohx;

namespace {

struct Loaded {
  Forest f;
  VisitForest vf;
};
Loaded load(const void* model, uint64_t len) {
  Loaded l;
  l.f = load_model_buffer(model, (size_t)len);
  l.f.validate();
  l.vf = emit_visits(l.f, place_forest(l.f, LayoutParams()));
  return l;
}

}  // namespace

// tree_offsets and leaf_offset: ntree + 1 entries each; leaf_node: the file node of every leaf counter
extern "C" __attribute__((visibility("default"))) int ohx_visits_layout(const void* model, uint64_t len, uint64_t cap_trees,
                                                                       uint64_t cap_leaves, uint64_t* ntree,
                                                                       uint64_t* tree_offsets, uint32_t* leaf_offset,
                                                                       uint32_t* leaf_node) {
  try {
    const Loaded l = load(model, len);
    const uint64_t T = l.f.trees.size();
    *ntree = T;
    if (T > cap_trees || l.vf.leaf_node.size() > cap_leaves) throw OhxError("ohx_visits_layout: the arrays are too small");
    memcpy(tree_offsets, l.vf.tree_offsets.data(), (T + 1) * sizeof(uint64_t));
    memcpy(leaf_offset, l.vf.leaf_offset.data(), (T + 1) * sizeof(uint32_t));
    if (!l.vf.leaf_node.empty()) memcpy(leaf_node, l.vf.leaf_node.data(), l.vf.leaf_node.size() * sizeof(uint32_t));
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

extern "C" __attribute__((visibility("default"))) int ohx_visits_node_sums(const void* model, uint64_t len,
                                                                          const uint64_t* leaf_counts, uint64_t nleaf,
                                                                          uint64_t* node_counts, uint64_t nnode) {
  try {
    const Loaded l = load(model, len);
    if (nleaf != l.vf.leaf_node.size() || nnode != l.vf.tree_offsets.back())
      throw OhxError("ohx_visits_node_sums: the booster has " + std::to_string(l.vf.leaf_node.size()) + " leaves and " +
                     std::to_string(l.vf.tree_offsets.back()) + " nodes");
    visit_node_sums(l.f, l.vf, leaf_counts, node_counts);
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// The covers OHXBoosterRefreshCover would store for these node counts, tree after tree in file numbering.  A refusal
// returns -1 and sum_hess holds the forest's covers as they are afterwards: unchanged.
extern "C" __attribute__((visibility("default"))) int ohx_visits_refresh(const void* model, uint64_t len,
                                                                        const uint64_t* node_counts, uint64_t nnode,
                                                                        float prior_weight, float* sum_hess) {
  try {
    Loaded l = load(model, len);
    if (nnode != l.vf.tree_offsets.back()) throw OhxError("ohx_visits_refresh: the booster has " + std::to_string(l.vf.tree_offsets.back()) + " nodes");
    int rc = 0;
    try {
      std::vector<std::vector<float>> covers = refreshed_covers(l.f, l.vf, node_counts, prior_weight);
      for (size_t t = 0; t < covers.size(); ++t) l.f.trees[t].sum_hess = std::move(covers[t]);
    } catch (const OhxError& e) {
      synth_set_error(e.what());
      rc = -1;
    }
    for (size_t t = 0; t < l.f.trees.size(); ++t)
      memcpy(sum_hess + l.vf.tree_offsets[t], l.f.trees[t].sum_hess.data(), l.f.trees[t].size() * sizeof(float));
    return rc;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// takes_lds[t] = 1 where tree t keeps its histogram in LDS.  info: [0] rows staged in LDS, [1] words of a block's
// histogram, [2] / [3] dynamic LDS bytes of the LDS / the global kernel, [4] the capacity in leaves at this feature
// count, [5] / [6] blocks (x) of the LDS / the global kernel for `ntiles` tiles on `num_cus` CUs, [7] trees on the LDS path
extern "C" __attribute__((visibility("default"))) int ohx_visits_plan(const void* model, uint64_t len, uint32_t lds_leaves,
                                                                     int force_global, int num_cus, uint64_t ntiles,
                                                                     uint8_t* takes_lds, uint64_t info[8]) {
  try {
    const Loaded l = load(model, len);
    const VisitPlan p = plan_visits(l.vf, l.f.num_feature, lds_leaves, force_global != 0);
    for (size_t t = 0; t < l.f.trees.size(); ++t) takes_lds[t] = 0;
    for (uint32_t t : p.lds_trees) takes_lds[t] = 1;
    info[0] = p.stage ? 1 : 0;
    info[1] = p.hist_leaves;
    info[2] = p.lds_bytes_lds;
    info[3] = p.lds_bytes_global;
    info[4] = visit_lds_capacity(l.f.num_feature);
    info[5] = visit_lds_blocks(ntiles, num_cus);
    info[6] = visit_global_blocks(ntiles, num_cus);
    info[7] = p.lds_trees.size();
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}
