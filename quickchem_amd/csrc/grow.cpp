// Host side of the tree grower (grow.hpp): the quantile cuts, the cut checks, the features of a tree, the assembly of a
// Tree from the device's node records and the launch plan.  No device code: libohx_synth.so links it too, for the
// tests that need no GPU.
#include "grow.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>

namespace ohx {

uint64_t quantile_cuts(const float* data, uint64_t nrow, uint64_t ncol, float missing, int max_bins, uint64_t* cut_ptr,
                       float* cut_values, uint64_t cap) {
  const bool missing_is_nan = missing != missing;
  uint64_t total = 0;
  std::vector<float> s, cuts;
  cut_ptr[0] = 0;
  for (uint64_t c = 0; c < ncol; ++c) {
    s.clear();
    for (uint64_t r = 0; r < nrow; ++r) {
      const float v = data[r * ncol + c];
      if (v != v || (!missing_is_nan && v == missing) || !std::isfinite(v)) continue;
      s.push_back(v);
    }
    std::sort(s.begin(), s.end());
    cuts.clear();
    const uint64_t n = s.size();
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; ++i)
      if (i == 0 || s[i] != s[i - 1]) ++m;
    if (m >= 2 && m <= (uint64_t)max_bins) {
      for (uint64_t i = 1; i < n; ++i)
        if (s[i] != s[i - 1]) cuts.push_back(s[i]);
    } else if (m > (uint64_t)max_bins) {
      for (uint64_t j = 1; j < (uint64_t)max_bins; ++j) {
        const float v = s[(size_t)(j * n / (uint64_t)max_bins)];
        if (v == s[0] || (!cuts.empty() && v == cuts.back())) continue;
        cuts.push_back(v);
      }
    }
    for (size_t i = 0; i < cuts.size(); ++i)
      if (total + i < cap) cut_values[total + i] = cuts[i];
    total += cuts.size();
    cut_ptr[c + 1] = total;
  }
  return total;
}

void grow_check_cuts(const uint64_t* cut_ptr, const float* cut_values, uint32_t num_feature, const char* what) {
  if (cut_ptr[0] != 0) throw OhxError(std::string(what) + ": cut_ptr[0] must be 0");
  for (uint32_t f = 0; f < num_feature; ++f) {
    if (cut_ptr[f + 1] < cut_ptr[f]) throw OhxError(std::string(what) + ": cut_ptr must not descend (feature " + std::to_string(f) + ")");
    const uint64_t n = cut_ptr[f + 1] - cut_ptr[f];
    if (n > kGrowMaxCuts)
      throw OhxError(std::string(what) + ": feature " + std::to_string(f) + " has " + std::to_string(n) +
                     " cuts; at most 254 fit the uint8 bins");
    for (uint64_t j = cut_ptr[f]; j < cut_ptr[f + 1]; ++j) {
      if (!std::isfinite(cut_values[j]))
        throw OhxError(std::string(what) + ": the cuts of feature " + std::to_string(f) + " are not all finite");
      if (j > cut_ptr[f] && !(cut_values[j - 1] < cut_values[j]))
        throw OhxError(std::string(what) + ": the cuts of feature " + std::to_string(f) + " are not strictly ascending");
    }
  }
}

uint32_t grow_pick_features(uint64_t seed, uint64_t i, uint32_t F, float colsample, uint8_t* out) {
  const uint32_t n_sel = F <= kGrowMaxFeatures ? grow_num_selected(F, colsample) : 0;
  if (n_sel == 0) return 0;
  if (n_sel == F) {
    for (uint32_t f = 0; f < F; ++f) out[f] = (uint8_t)f;
    return n_sel;
  }
  const uint64_t key = grow_col_key(seed, i);
  std::pair<uint64_t, uint32_t> c[kGrowMaxFeatures];
  for (uint32_t f = 0; f < F; ++f) c[f] = {grow_mix(key + f), f};
  std::sort(c, c + F);   // by (c_f, f)
  bool in[kGrowMaxFeatures] = {};
  for (uint32_t k = 0; k < n_sel; ++k) in[c[k].second] = true;
  uint32_t k = 0;
  for (uint32_t f = 0; f < F; ++f)
    if (in[f]) out[k++] = (uint8_t)f;
  return n_sel;
}

namespace {

// the `take` entries of list[0 .. n) smallest by (mix(key + f), f), in the list's order
void pick_by_key(uint64_t key, const uint8_t* list, uint32_t n, uint32_t take, uint8_t* out) {
  std::pair<std::pair<uint64_t, uint32_t>, uint32_t> c[kGrowMaxFeatures];   // ((key, f), position)
  for (uint32_t k = 0; k < n; ++k) c[k] = {{grow_mix(key + list[k]), list[k]}, k};
  std::sort(c, c + n);
  bool in[kGrowMaxFeatures] = {};
  for (uint32_t k = 0; k < take; ++k) in[c[k].second] = true;
  uint32_t at = 0;
  for (uint32_t k = 0; k < n; ++k)
    if (in[k]) out[at++] = list[k];
}

}  // namespace

uint32_t grow_pick_level_features(uint64_t seed, uint64_t i, uint32_t d, const uint8_t* tree_list, uint32_t n_sel, float bylevel,
                                  uint8_t* out) {
  const uint32_t n_lvl = n_sel <= kGrowMaxFeatures ? grow_num_selected(n_sel, bylevel) : 0;
  if (n_lvl == 0) return 0;
  if (n_lvl == n_sel) std::copy(tree_list, tree_list + n_sel, out);
  else pick_by_key(grow_level_key(grow_col_key(seed, i), d), tree_list, n_sel, n_lvl, out);
  return n_lvl;
}

uint32_t grow_pick_node_features(uint64_t seed, uint64_t i, uint32_t p, const uint8_t* level_list, uint32_t n_lvl, float bynode,
                                 uint8_t* out) {
  const uint32_t n_node = n_lvl <= kGrowMaxFeatures ? grow_num_selected(n_lvl, bynode) : 0;
  if (n_node == 0) return 0;
  if (n_node == n_lvl) std::copy(level_list, level_list + n_lvl, out);
  else pick_by_key(grow_node_key(grow_col_key(seed, i), p), level_list, n_lvl, n_node, out);
  return n_node;
}

bool grow_interact_parse(const char* value, std::vector<uint64_t>* words) {
  if (value == nullptr || words == nullptr) return false;
  std::vector<uint64_t> w;
  const char* p = value;
  auto blanks = [&]() {
    while (*p == ' ' || *p == '\t') ++p;
  };
  blanks();
  if (*p++ != '[') return false;
  blanks();
  if (*p != ']') {
    for (;;) {   // a group
      if (*p++ != '[') return false;
      if (w.size() == 2 * (size_t)kGrowMaxGroups) return false;
      uint64_t g[2] = {0, 0};
      for (;;) {   // an id
        blanks();
        if (*p < '0' || *p > '9') return false;
        uint32_t f = 0;
        while (*p >= '0' && *p <= '9') {
          f = f * 10 + (uint32_t)(*p++ - '0');
          if (f >= kGrowMaxFeatures) return false;
        }
        if (grow_interact_has(g, f)) return false;
        g[f >> 6] |= 1ull << (f & 63u);
        blanks();
        if (*p == ']') break;
        if (*p++ != ',') return false;
      }
      ++p;
      w.push_back(g[0]);
      w.push_back(g[1]);
      blanks();
      if (*p == ']') break;
      if (*p++ != ',') return false;
      blanks();
    }
  }
  ++p;
  blanks();
  if (*p != '\0') return false;
  words->swap(w);
  return true;
}

bool grow_interact_active(const uint64_t* groups, uint32_t ngroups, uint32_t F) {
  uint64_t all[2];
  grow_interact_all(F < kGrowMaxFeatures ? F : kGrowMaxFeatures, all);
  for (uint32_t g = 0; g < ngroups; ++g)
    if ((all[0] & ~groups[2 * g]) == 0 && (all[1] & ~groups[2 * g + 1]) == 0) return false;
  return ngroups != 0;
}

Tree grow_assemble_tree(const GrowNode* nodes, uint32_t n, uint32_t num_feature, uint32_t max_nodes) {
  if (n == 0 || n > max_nodes || n % 2 == 0) throw OhxError("grown tree: " + std::to_string(n) + " nodes is not a tree");
  Tree t;
  t.resize(n);
  t.num_feature = (int32_t)num_feature;
  uint32_t next = 1;
  for (uint32_t i = 0; i < n; ++i) {
    const GrowNode& r = nodes[i];
    if (r.left >= 0) {
      // allocation order: a split takes the next two ids
      if ((uint32_t)r.left != next || r.right != r.left + 1 || (uint32_t)r.right >= n || r.feature >= num_feature)
        throw OhxError("grown tree: node " + std::to_string(i) + " is out of allocation order");
      if (nodes[r.left].parent != (int32_t)(i | 0x80000000u) || nodes[r.right].parent != (int32_t)i)
        throw OhxError("grown tree: the children of node " + std::to_string(i) + " do not name it");
      next += 2;
    } else if (r.right != -1) {
      throw OhxError("grown tree: node " + std::to_string(i) + " has one child");
    }
    t.left[i] = r.left;
    t.right[i] = r.right;
    t.parent[i] = i == 0 ? -1 : r.parent;
    t.feature[i] = r.left >= 0 ? r.feature : 0u;
    t.default_left[i] = r.left >= 0 ? (uint8_t)(r.default_left != 0) : (uint8_t)0;
    t.value[i] = r.value;
    t.deleted[i] = 0;
    t.loss_chg[i] = r.left >= 0 ? r.loss_chg : 0.0f;
    t.sum_hess[i] = r.sum_hess;
    t.base_weight[i] = r.base_weight;
    t.leaf_child_cnt[i] = 0;
  }
  if (next != n) throw OhxError("grown tree: " + std::to_string(n) + " records hold " + std::to_string(next) + " nodes");
  return t;
}

namespace {

// the plan for histograms of pair_bytes a (node, feature) pair in LDS
GrowPlan plan_grow_pairs(uint64_t nrow, uint32_t num_feature, uint64_t ncuts, int max_depth, int num_cus, uint32_t pair_bytes) {
  const uint32_t max_pairs = kGrowLdsBytes / pair_bytes;
  GrowPlan p;
  const uint64_t cus = num_cus > 0 ? (uint64_t)num_cus : 1;
  const uint64_t want = (nrow + kGrowBlock - 1) / kGrowBlock, cap = cus * kGrowRowBlocksPerCu;
  p.row_blocks = (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
  p.bin_lds_bytes = (uint32_t)(ncuts * sizeof(float));
  p.bins_bytes = (uint64_t)num_feature * nrow;
  const uint32_t F = std::max<uint32_t>(num_feature, 1);
  for (int d = 0; d < max_depth; ++d) {
    GrowLevelPlan l;
    l.slots = 1u << d;
    // all of a level's nodes in one block where they fit, then as many features as LDS still holds: a block reads pos,
    // pred and the label of every row once per group, and the bins of its own features only
    l.node_group = std::min(l.slots, max_pairs);
    l.feat_group = std::max(1u, std::min(F, max_pairs / l.node_group));
    l.node_groups = (l.slots + l.node_group - 1) / l.node_group;
    l.feat_groups = (F + l.feat_group - 1) / l.feat_group;
    l.feat_group = (F + l.feat_groups - 1) / l.feat_groups;     // the same number of groups, evenly filled
    l.lds_bytes = l.node_group * l.feat_group * pair_bytes;
    const uint64_t groups = (uint64_t)l.node_groups * l.feat_groups;
    const uint64_t hwant = (nrow + kGrowHistBlock - 1) / kGrowHistBlock;
    const uint64_t hcap = std::max<uint64_t>(1, cus * kGrowHistBlocksPerCu / groups);
    // (one block's trips stay below kGrowMaxTrips at 2^31 rows whatever the cap: 2^31 / 1024 = 2^21)
    l.hist_blocks = (uint32_t)std::max<uint64_t>(1, std::min(hwant, hcap));
    p.levels.push_back(l);
    p.hist_bytes = (uint64_t)l.slots * F * kGrowBins * 16;
  }
  return p;
}

}  // namespace

GrowPlan plan_grow(uint64_t nrow, uint32_t num_feature, uint64_t ncuts, int max_depth, int num_cus) {
  return plan_grow_pairs(nrow, num_feature, ncuts, max_depth, num_cus, kGrowPairBytes);
}

GrowPlan plan_grow_weighted(uint64_t nrow, uint32_t num_feature, uint64_t ncuts, int max_depth, int num_cus) {
  GrowPlan p = plan_grow_pairs(nrow, num_feature, ncuts, max_depth, num_cus, kGrowWeightedPairBytes);
  p.pairs_bytes = grow_pair_plane_bytes(nrow);   // allocated only where the pair path runs
  return p;
}

GrowDeepPlan plan_grow_deep(uint64_t nrow, uint32_t num_feature, uint64_t ncuts, int max_depth, int num_cus) {
  GrowDeepPlan p;
  p.lds = plan_grow_weighted(nrow, num_feature, ncuts, std::min(max_depth, kGrowMaxDepth), num_cus);
  p.batch = kGrowDeepBatch;
  // a row per lane in natural order, as the other streaming kernels: a block outside the batch costs one load a row
  p.hist_blocks = p.lds.row_blocks;
  p.node_stride = grow_deep_node_stride(nrow, max_depth);
  const uint64_t F = std::max<uint32_t>(num_feature, 1);
  const uint64_t open = grow_deep_max_open(nrow, max_depth);
  if (max_depth > kGrowMaxDepth) p.scratch_bytes = std::min<uint64_t>(p.batch, open) * F * kGrowBins * 16;
  // (the levels in LDS index `best` by 2^d slots, whatever the rows)
  p.best_bytes = std::max<uint64_t>(open, 1ull << (std::min(max_depth, kGrowMaxDepth) - 1)) * F * sizeof(GrowCand);
  return p;
}

GrowDeepPlan plan_grow_deep_sampled(uint64_t nrow, uint32_t num_feature, uint32_t n_sel, uint64_t ncuts, int max_depth, int num_cus) {
  GrowDeepPlan p = plan_grow_deep(nrow, n_sel, ncuts, max_depth, num_cus);
  p.lds.bins_bytes = (uint64_t)num_feature * nrow;   // the bins hold every feature
  return p;
}

uint32_t plan_grow_eval_blocks(uint64_t nrow, int num_cus) {
  const uint64_t cus = num_cus > 0 ? (uint64_t)num_cus : 1;
  const uint64_t want = (nrow + kGrowBlock - 1) / kGrowBlock, cap = cus * kGrowRowBlocksPerCu;
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

double grow_sum_rmse(GrowSum s, uint64_t n) {
  s = grow_sum_normal(s);
  const unsigned __int128 S = ((unsigned __int128)s.hi << 32) + (unsigned __int128)s.lo;
  return std::sqrt((double)S * (1.0 / 281474976710656.0) / (double)n);
}

double grow_wide_rmse(GrowWideSum s, uint64_t W) {
  const unsigned __int128 S = grow_wide_value(s);
  return std::sqrt(((double)S * (1.0 / 4722366482869645213696.0)) / ((double)(unsigned __int128)W * (1.0 / 16777216.0)));
}

double grow_wide_mean(GrowWideSum s, uint64_t W) {
  const unsigned __int128 S = grow_wide_value(s);
  return ((double)S * (1.0 / 281474976710656.0)) / ((double)(unsigned __int128)W * (1.0 / 16777216.0));
}

double grow_wide_quantile(GrowWideSum s, uint64_t W) {
  const unsigned __int128 S = grow_wide_value(s);
  return ((double)S * (1.0 / 4722366482869645213696.0)) / ((double)(unsigned __int128)W * (1.0 / 16777216.0));
}

}  // namespace ohx
