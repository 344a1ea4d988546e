// Host side of the node visit counts (visits.hpp): the walk's node format, leaf counters to node sums, the refreshed
// covers and the launch plan.  No device code: libohx_synth.so links it too, for the tests that need no GPU.
#include "visits.hpp"

#include <cmath>
#include <string>

namespace ohx {

VisitForest emit_visits(const Forest& f, const Placement& p) {
  if (p.num_slots * sizeof(VisitNode) >= 0xFFFFFFF0ull) throw OhxError("booster too large for the visit-count node format (4 GiB of nodes)");
  VisitForest out;
  const size_t T = f.trees.size();
  out.nodes.assign((size_t)p.num_slots, VisitNode{0.0f, 0u, 0u, 0u});
  out.roots = p.roots;
  out.leaf_offset.assign(T + 1, 0u);
  out.tree_offsets.assign(T + 1, 0u);
  for (size_t ti = 0; ti < T; ++ti) {
    const Tree& t = f.trees[ti];
    const auto& slot = p.slot_of[ti];
    uint32_t leaves = 0;
    for (size_t i = 0; i < t.size(); ++i) {
      if (slot[i] == kNoSlot) continue;
      VisitNode nd{t.value[i], 0u, 0u, 0u};
      if (t.left[i] == -1) {
        nd.leaf = leaves++;
        out.leaf_node.push_back((uint32_t)i);
      } else {
        const uint32_t ls = slot[(size_t)t.left[i]], rs = slot[(size_t)t.right[i]];
        if (rs != ls + 1) throw OhxError("internal error: placement broke sibling adjacency");
        nd.left = ls;
        nd.feat_dl = t.feature[i] | ((uint32_t)(t.default_left[i] ? 1u : 0u) << 31);
      }
      out.nodes[slot[i]] = nd;
    }
    if ((uint64_t)out.leaf_offset[ti] + leaves > 0xFFFFFFFFull) throw OhxError("booster has too many leaves for the visit counters");
    out.leaf_offset[ti + 1] = out.leaf_offset[ti] + leaves;
    out.tree_offsets[ti + 1] = out.tree_offsets[ti] + t.size();
  }
  return out;
}

namespace {

// the nodes of tree t reachable from its root, parents before children
std::vector<int32_t> reachable_order(const Tree& t) {
  std::vector<int32_t> order;
  if (t.size() == 0) return order;
  order.push_back(0);
  for (size_t k = 0; k < order.size(); ++k) {
    const int32_t n = order[k];
    if (t.left[(size_t)n] != -1) {
      order.push_back(t.left[(size_t)n]);
      order.push_back(t.right[(size_t)n]);
    }
  }
  return order;
}

}  // namespace

void visit_node_sums(const Forest& f, const VisitForest& vf, const uint64_t* leaf_counts, uint64_t* node_counts) {
  for (size_t ti = 0; ti < f.trees.size(); ++ti) {
    const Tree& t = f.trees[ti];
    uint64_t* out = node_counts + vf.tree_offsets[ti];
    for (size_t i = 0; i < t.size(); ++i) out[i] = 0;
    for (uint32_t l = vf.leaf_offset[ti]; l < vf.leaf_offset[ti + 1]; ++l) out[vf.leaf_node[l]] = leaf_counts[l];
    const std::vector<int32_t> order = reachable_order(t);
    for (size_t k = order.size(); k-- > 0;) {
      const size_t n = (size_t)order[k];
      if (t.left[n] != -1) out[n] = out[(size_t)t.left[n]] + out[(size_t)t.right[n]];
    }
  }
}

std::vector<std::vector<float>> refreshed_covers(const Forest& f, const VisitForest& vf, const uint64_t* node_counts,
                                                 float prior_weight) {
  std::vector<std::vector<float>> out(f.trees.size());
  uint64_t splits = 0, bad = 0;
  size_t bad_tree = 0, bad_node = 0;
  float bad_value = 0.0f;
  for (size_t ti = 0; ti < f.trees.size(); ++ti) {
    const Tree& t = f.trees[ti];
    out[ti] = t.sum_hess;
    const uint64_t* cnt = node_counts + vf.tree_offsets[ti];
    std::vector<int32_t> order = reachable_order(t);
    for (int32_t n32 : order) {
      const size_t n = (size_t)n32;
      // two roundings, never a fused multiply-add (the translation unit is built with -ffp-contract=off)
      const float prior = prior_weight * t.sum_hess[n];
      const float cover = (float)cnt[n] + prior;
      out[ti][n] = cover;
      if (t.left[n] == -1) continue;
      ++splits;
      if (!(std::isfinite(cover) && cover > 0.0f)) {
        if (bad == 0 || ti < bad_tree || (ti == bad_tree && n < bad_node)) bad_tree = ti, bad_node = n, bad_value = cover;
        ++bad;
      }
    }
  }
  if (bad != 0)
    throw OhxError("OHXBoosterRefreshCover: the split at node " + std::to_string(bad_node) + " of tree " +
                   std::to_string(bad_tree) + " would get cover " + std::to_string(bad_value) + " (" + std::to_string(bad) +
                   " of " + std::to_string(splits) + " splits would not have a finite cover > 0: no counted row reached them); "
                   "the covers are unchanged.  A prior_weight > 0 blends the old cover in and keeps such subtrees positive");
  return out;
}

VisitPlan plan_visits(const VisitForest& vf, uint32_t num_feature, uint32_t lds_leaves, bool force_global) {
  VisitPlan p;
  p.stage = visit_stages(num_feature);
  const size_t tiles = p.stage ? visit_tile_bytes(num_feature) : 0;
  uint32_t cap = visit_lds_capacity(num_feature);
  if (lds_leaves != 0 && lds_leaves < cap) cap = lds_leaves;
  const uint32_t T = (uint32_t)(vf.leaf_offset.size() - 1);
  for (uint32_t t = 0; t < T; ++t) {
    const uint32_t n = vf.leaves(t);
    if (!force_global && n <= cap) {
      p.lds_trees.push_back(t);
      if (n > p.hist_leaves) p.hist_leaves = n;
    } else {
      p.global_trees.push_back(t);
    }
  }
  p.lds_bytes_lds = tiles + (size_t)p.hist_leaves * sizeof(uint32_t);
  p.lds_bytes_global = tiles;
  return p;
}

}  // namespace ohx
