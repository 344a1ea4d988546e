// Host side of the leaf refit (refit.hpp): the solve on a leaf's sums, the leaf tables of a forest and the launch plan.
// No device code: libohx_synth.so links it too, for the tests that need no GPU.
#include "refit.hpp"

namespace ohx {

uint64_t refit_solve(const int64_t* G, const uint64_t* H, uint64_t n, float eta, float lambda, int unvisited, float* value,
                     float* base_weight) {
  uint64_t refit = 0;
  for (uint64_t l = 0; l < n; ++l) {
    if (H[l] == 0) {
      if (unvisited != 0) value[l] = base_weight[l] = 0.0f;
      continue;
    }
    refit_solve_leaf(G[l], H[l], eta, lambda, &value[l], &base_weight[l]);
    ++refit;
  }
  return refit;
}

void refit_gather_leaves(const Forest& f, const VisitForest& vf, float* value, float* base_weight) {
  for (size_t t = 0; t < f.trees.size(); ++t)
    for (uint32_t l = vf.leaf_offset[t]; l < vf.leaf_offset[t + 1]; ++l) {
      value[l] = f.trees[t].value[vf.leaf_node[l]];
      base_weight[l] = f.trees[t].base_weight[vf.leaf_node[l]];
    }
}

void refit_write_back(Forest& f, const VisitForest& vf, const float* value, const float* base_weight) {
  for (size_t t = 0; t < f.trees.size(); ++t)
    for (uint32_t l = vf.leaf_offset[t]; l < vf.leaf_offset[t + 1]; ++l) {
      f.trees[t].value[vf.leaf_node[l]] = value[l];
      f.trees[t].base_weight[vf.leaf_node[l]] = base_weight[l];
    }
}

RefitPlan plan_refit(uint64_t nrow, uint32_t num_feature, uint64_t ntree, int num_cus) {
  RefitPlan p;
  p.stage = visit_stages(num_feature);
  p.lds_bytes = p.stage ? visit_tile_bytes(num_feature) : 0;
  const uint64_t cus = num_cus > 0 ? (uint64_t)num_cus : 1;
  const uint64_t tiles = (nrow + 63) / 64, waves = kRefitBlock / 64;
  const uint64_t want_ids = (tiles + waves - 1) / waves, want_accum = (nrow + kRefitBlock - 1) / kRefitBlock;
  const uint64_t cap_ids = cus * kRefitIdsBlocksPerCu, cap_accum = cus * kRefitAccumBlocksPerCu;
  p.ids_blocks = (uint32_t)(want_ids < cap_ids ? want_ids : cap_ids);
  p.accum_blocks = (uint32_t)(want_accum < cap_accum ? want_accum : cap_accum);
  p.ids_bytes = ntree * nrow * sizeof(uint32_t);
  return p;
}

}  // namespace ohx
