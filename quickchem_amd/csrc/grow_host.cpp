// Test support (libohx_synth.so): the host pieces of the tree grower (grow.hpp) without a GPU - the split choice on
// injected histograms (the shared grow_best_split the split kernel runs per lane), the assembly of a tree from node
// records appended to a booster and written in a file format, and the launch plan.  The product library runs the same
// functions of grow.cpp behind OHXBoosterBoostTrees; and the host pieces of the held-out metric behind
// OHXBoosterBoostTreesEval: the comparison of two sums, the stop rule, the RMSE of a sum and the launch shape.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "grow.hpp"
#include "grow_quantile.hpp"

namespace ohx {
void synth_set_error(const std::string& m);   // synth_host.cpp
}

using namespace ohx;

namespace {

// a plan as the ohx_grow_plan* exports hand it out: info[0 .. 7] and max_depth x 7 level figures
void write_plan(const GrowPlan& p, uint64_t bins_bytes, uint32_t pair_bytes, uint64_t* info, uint64_t* levels) {
  info[0] = p.row_blocks;
  info[1] = kGrowBlock;
  info[2] = p.bin_lds_bytes;
  info[3] = bins_bytes;
  info[4] = p.hist_bytes;
  info[5] = kGrowHistBlock;
  info[6] = kGrowLdsBytes / pair_bytes;
  info[7] = pair_bytes;
  for (size_t d = 0; d < p.levels.size(); ++d) {
    const GrowLevelPlan& l = p.levels[d];
    const uint64_t v[7] = {l.slots, l.node_group, l.feat_group, l.node_groups, l.feat_groups, l.hist_blocks, l.lds_bytes};
    memcpy(levels + d * 7, v, sizeof v);
  }
}

}  // namespace

// G / H: [num_feature][256].  out: [0] valid, [1] feature, [2] j, [3] default_left, [4] splits (valid and
// loss_chg > gamma); sums: [0] GL, [1] HL
extern "C" __attribute__((visibility("default"))) int ohx_grow_node_split(const int64_t* G, const uint64_t* H,
                                                                         uint32_t num_feature, const uint64_t* cut_ptr,
                                                                         int64_t Gp, uint64_t Hp, float lambda, float gamma,
                                                                         uint64_t min_child_rows, double* loss_chg,
                                                                         uint32_t out[5], int64_t sums[2]) {
  try {
    const GrowCand c = grow_node_split(G, H, num_feature, cut_ptr, Gp, Hp, lambda, GrowCountHess{min_child_rows});
    *loss_chg = c.loss_chg;
    out[0] = c.valid;
    out[1] = c.key >> 9;
    out[2] = (c.key >> 1) & 255u;
    out[3] = c.key & 1u;
    out[4] = c.valid && c.loss_chg > (double)gamma ? 1u : 0u;
    sums[0] = c.GL;
    sums[1] = (int64_t)c.HL;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// One tree of n node records, given as arrays, is assembled (grow_assemble_tree) and appended to the booster of
// `model`; the longer forest comes back in `format` (0 legacy binary, 1 JSON, 2 UBJSON; free with ohx_synth_free).
extern "C" __attribute__((visibility("default"))) int ohx_grow_append(const void* model, uint64_t len, uint32_t n,
                                                                     const int32_t* left, const int32_t* right,
                                                                     const int32_t* parent, const uint32_t* feature,
                                                                     const uint32_t* default_left, const float* value,
                                                                     const float* loss_chg, const float* sum_hess,
                                                                     const float* base_weight, int format, uint8_t** out_buf,
                                                                     uint64_t* out_len) {
  try {
    Forest f = load_model_buffer(model, (size_t)len);
    f.validate();
    std::vector<GrowNode> nodes(n);
    for (uint32_t i = 0; i < n; ++i) {
      GrowNode& r = nodes[i];
      r.G = 0;
      r.H = 0;
      r.left = left[i];
      r.right = right[i];
      r.parent = parent[i];
      r.feature = feature[i];
      r.cut = 0;
      r.default_left = default_left[i];
      r.value = value[i];
      r.loss_chg = loss_chg[i];
      r.sum_hess = sum_hess[i];
      r.base_weight = base_weight[i];
    }
    f.trees.push_back(grow_assemble_tree(nodes.data(), n, f.num_feature));
    f.tree_info.push_back(0);
    f.validate();
    std::vector<uint8_t> b;
    if (format == 1) {
      const std::string s = write_json_model(f);
      b.assign(s.begin(), s.end());
    } else {
      b = format == 2 ? write_ubjson_model(f) : write_legacy_binary(f);
    }
    *out_buf = (uint8_t*)malloc(b.size() ? b.size() : 1);
    memcpy(*out_buf, b.data(), b.size());
    *out_len = b.size();
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// info: [0] blocks of the bin, partition and leaf kernels, [1] rows such a block takes per trip, [2] LDS bytes of the
// staged cuts, [3] bytes of the bin planes, [4] bytes of the deepest level's global histograms, [5] rows a histogram
// block takes per trip, [6] (node, feature) histograms a block's LDS holds at most, [7] LDS bytes of one of them.
// levels: max_depth x 7 = slots, node_group, feat_group, node_groups, feat_groups, hist_blocks, lds_bytes
extern "C" __attribute__((visibility("default"))) int ohx_grow_plan(uint64_t nrow, uint32_t num_feature, uint64_t ncuts,
                                                                   int max_depth, int num_cus, uint64_t info[8],
                                                                   uint64_t* levels) {
  try {
    if (max_depth < 1 || max_depth > kGrowMaxDepth) throw OhxError("ohx_grow_plan: max_depth must be in 1..8");
    write_plan(plan_grow(nrow, num_feature, ncuts, max_depth, num_cus), (uint64_t)num_feature * nrow, kGrowPairBytes, info, levels);
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// ---- the held-out metric ----

// sums: n pairs (hi, lo), the held-out sums after 0 .. n - 1 trees.  out: [0] rounds_run, [1] best_round
extern "C" __attribute__((visibility("default"))) int ohx_grow_eval_stop(const uint64_t* sums, uint32_t n, int patience,
                                                                        uint32_t out[2]) {
  try {
    if (n == 0) throw OhxError("ohx_grow_eval_stop: no sums");
    if (patience < 0) throw OhxError("ohx_grow_eval_stop: patience must be >= 0");
    std::vector<GrowSum> S(n);
    for (uint32_t t = 0; t < n; ++t) {
      S[t].hi = sums[2 * t];
      S[t].lo = sums[2 * t + 1];
    }
    grow_eval_stop(S.data(), n - 1, patience, &out[0], &out[1]);
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// -1 / 0 / 1 as a < b, a == b, a > b; normal: a's (hi, lo) with lo < 2^32
extern "C" __attribute__((visibility("default"))) int ohx_grow_eval_compare(const uint64_t a[2], const uint64_t b[2],
                                                                           uint64_t normal[2]) {
  GrowSum x, y;
  x.hi = a[0];
  x.lo = a[1];
  y.hi = b[0];
  y.lo = b[1];
  const GrowSum nx = grow_sum_normal(x);
  normal[0] = nx.hi;
  normal[1] = nx.lo;
  return grow_sum_less(x, y) ? -1 : grow_sum_less(y, x) ? 1 : 0;
}

extern "C" __attribute__((visibility("default"))) double ohx_grow_eval_rmse(uint64_t hi, uint64_t lo, uint64_t n) {
  GrowSum s;
  s.hi = hi;
  s.lo = lo;
  return grow_sum_rmse(s, n);
}

// info: [0] blocks of grow_sse_kernel and grow_walk_sse_kernel over nrow rows, [1] rows such a block takes per trip
extern "C" __attribute__((visibility("default"))) int ohx_grow_eval_plan(uint64_t nrow, int num_cus, uint64_t info[2]) {
  info[0] = plan_grow_eval_blocks(nrow, num_cus);
  info[1] = kGrowBlock;
  return 0;
}

// ---- row weights ----

// ohx_grow_node_split over fixed-point hessian histograms (the GrowFixedHess policy); sums[1] is HL in fixed point
extern "C" __attribute__((visibility("default"))) int ohx_grow_node_split_weighted(const int64_t* G, const uint64_t* H,
                                                                                  uint32_t num_feature, const uint64_t* cut_ptr,
                                                                                  int64_t Gp, uint64_t Hp, float lambda, float gamma,
                                                                                  float min_child_weight, double* loss_chg,
                                                                                  uint32_t out[5], uint64_t sums[2]) {
  try {
    const GrowCand c = grow_node_split(G, H, num_feature, cut_ptr, Gp, Hp, lambda, GrowFixedHess{(double)min_child_weight});
    *loss_chg = c.loss_chg;
    out[0] = c.valid;
    out[1] = c.key >> 9;
    out[2] = (c.key >> 1) & 255u;
    out[3] = c.key & 1u;
    out[4] = c.valid && c.loss_chg > (double)gamma ? 1u : 0u;
    sums[0] = (uint64_t)c.GL;
    sums[1] = c.HL;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// the weighted leaf solve: out[0] leaf value, out[1] base_weight, out[2] sum_hess
extern "C" __attribute__((visibility("default"))) void ohx_grow_solve_leaf_weighted(int64_t G, uint64_t H, float eta, float lambda,
                                                                                   float out[3]) {
  grow_solve_leaf_weighted(G, H, eta, lambda, &out[0], &out[1]);
  out[2] = (float)grow_hess(H);
}

// ohx_grow_plan by plan_grow_weighted
extern "C" __attribute__((visibility("default"))) int ohx_grow_plan_weighted(uint64_t nrow, uint32_t num_feature, uint64_t ncuts,
                                                                            int max_depth, int num_cus, uint64_t info[8],
                                                                            uint64_t* levels) {
  try {
    if (max_depth < 1 || max_depth > kGrowMaxDepth) throw OhxError("ohx_grow_plan_weighted: max_depth must be in 1..8");
    write_plan(plan_grow_weighted(nrow, num_feature, ncuts, max_depth, num_cus), (uint64_t)num_feature * nrow, kGrowWeightedPairBytes, info,
               levels);
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// s: (p2, p1, p0); W: the sum of hq
extern "C" __attribute__((visibility("default"))) double ohx_grow_weighted_rmse(const uint64_t s[3], uint64_t W) {
  GrowWideSum x;
  x.p2 = s[0];
  x.p1 = s[1];
  x.p0 = s[2];
  return grow_wide_rmse(x, W);
}

// -1 / 0 / 1 as a < b, a == b, a > b, as the exact integers p2 * 2^64 + p1 * 2^32 + p0
extern "C" __attribute__((visibility("default"))) int ohx_grow_weighted_compare(const uint64_t a[3], const uint64_t b[3]) {
  GrowWideSum x, y;
  x.p2 = a[0];
  x.p1 = a[1];
  x.p0 = a[2];
  y.p2 = b[0];
  y.p1 = b[1];
  y.p0 = b[2];
  return grow_sum_less(x, y) ? -1 : grow_sum_less(y, x) ? 1 : 0;
}

// the stop rule over n wide sums (p2, p1, p0).  out: [0] rounds_run, [1] best_round
extern "C" __attribute__((visibility("default"))) int ohx_grow_weighted_stop(const uint64_t* sums, uint32_t n, int patience,
                                                                            uint32_t out[2]) {
  try {
    if (n == 0) throw OhxError("ohx_grow_weighted_stop: no sums");
    if (patience < 0) throw OhxError("ohx_grow_weighted_stop: patience must be >= 0");
    std::vector<GrowWideSum> S(n);
    for (uint32_t t = 0; t < n; ++t) {
      S[t].p2 = sums[3 * t];
      S[t].p1 = sums[3 * t + 1];
      S[t].p0 = sums[3 * t + 2];
    }
    grow_eval_stop(S.data(), n - 1, patience, &out[0], &out[1]);
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// ---- row and column subsampling (OHXBoosterBoostTreesSampled) ----

// out[r] = 1 where row r is in the bag of tree `tree` (grow_row_key, grow_in_bag with grow_sample_threshold(subsample));
// *k_s: the threshold.  A subsample that is refused (k_s == 0) is an error.
extern "C" __attribute__((visibility("default"))) int ohx_grow_bag(uint64_t seed, uint64_t tree, uint64_t nrow, float subsample,
                                                                  uint8_t* out, uint32_t* k_s) {
  try {
    const uint32_t k = grow_sample_threshold(subsample);
    if (k == 0) throw OhxError("ohx_grow_bag: subsample must be finite, > 0 and <= 1, and rint(subsample * 2^24) >= 1");
    *k_s = k;
    const uint64_t key = grow_row_key(seed, tree);
    for (uint64_t r = 0; r < nrow; ++r) out[r] = k == kGrowSampleOne || grow_in_bag(key, r, k) ? 1 : 0;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// out[0 .. *n_sel): the features of tree `tree` (grow_pick_features); out holds F entries
extern "C" __attribute__((visibility("default"))) int ohx_grow_features(uint64_t seed, uint64_t tree, uint32_t F, float colsample,
                                                                       uint8_t* out, uint32_t* n_sel) {
  try {
    if (F == 0 || F > kGrowMaxFeatures) throw OhxError("ohx_grow_features: 1 to 128 features");
    const uint32_t n = grow_pick_features(seed, tree, F, colsample, out);
    if (n == 0) throw OhxError("ohx_grow_features: colsample_bytree must be finite, > 0 and <= 1");
    *n_sel = n;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// ---- column sampling by level and by node (docs/29_colsample_level_node.md) ----

// keys[0] = K_lvl(tree, level) and keys[1] = K_node(tree, node) of the draws (grow_col_key, grow_level_key, grow_node_key)
extern "C" __attribute__((visibility("default"))) void ohx_grow_colsample_keys(uint64_t seed, uint64_t tree, uint32_t level, uint32_t node,
                                                                              uint64_t keys[2]) {
  const uint64_t col = grow_col_key(seed, tree);
  keys[0] = grow_level_key(col, level);
  keys[1] = grow_node_key(col, node);
}

// out[0 .. *n_out): what level `level` (which == 0: grow_pick_level_features) or node `at` (which == 1:
// grow_pick_node_features) of tree `tree` keeps of list[0 .. n) at `fraction`; out holds n entries
extern "C" __attribute__((visibility("default"))) int ohx_grow_colsample_pick(int which, uint64_t seed, uint64_t tree, uint32_t at,
                                                                             const uint8_t* list, uint32_t n, float fraction,
                                                                             uint8_t* out, uint32_t* n_out) {
  try {
    if (n == 0 || n > kGrowMaxFeatures) throw OhxError("ohx_grow_colsample_pick: a list of 1 to 128 features");
    const uint32_t k = which == 0 ? grow_pick_level_features(seed, tree, at, list, n, fraction, out)
                                  : grow_pick_node_features(seed, tree, at, list, n, fraction, out);
    if (k == 0) throw OhxError("ohx_grow_colsample_pick: the fraction must be finite, > 0 and <= 1");
    *n_out = k;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// grow_node_has_feature: 1 where f is one of node `node`'s n_node features of list[0 .. n_lvl), by the rank a split kernel
// computes; f must be in the list
extern "C" __attribute__((visibility("default"))) int ohx_grow_colsample_has(uint64_t seed, uint64_t tree, uint32_t node,
                                                                            const uint8_t* list, uint32_t n_lvl, uint32_t n_node,
                                                                            uint32_t f) {
  return grow_node_has_feature(seed, tree, node, list, n_lvl, n_node, f) ? 1 : 0;
}

// ---- interaction constraints (docs/35_interaction_constraints.md) ----

// grow_interact_parse: the groups of `value` as words[0 .. 2 * *ngroups) (words holds 128), and *active =
// grow_interact_active for a booster of F features; -1 where the grammar refuses the value
extern "C" __attribute__((visibility("default"))) int ohx_grow_interact_parse(const char* value, uint32_t F, uint64_t* words,
                                                                             uint32_t* ngroups, int* active) {
  std::vector<uint64_t> w;
  if (!grow_interact_parse(value, &w)) {
    synth_set_error("ohx_grow_interact_parse: ohx_interaction_constraints is not a list of groups such as [[0,2],[1,3,4]]");
    return -1;
  }
  for (size_t k = 0; k < w.size(); ++k) words[k] = w[k];
  *ngroups = (uint32_t)(w.size() / 2);
  *active = grow_interact_active(w.data(), *ngroups, F) ? 1 : 0;
  return 0;
}

// grow_interact_allowed: out = A of a node whose path has split on the features P
extern "C" __attribute__((visibility("default"))) void ohx_grow_interact_allowed(const uint64_t P[2], const uint64_t* groups,
                                                                                uint32_t ngroups, uint32_t F, uint64_t out[2]) {
  grow_interact_allowed(P, groups, ngroups, F, out);
}

// the level plan of a sampled call: plan_grow_weighted over n_sel = grow_num_selected(num_feature, colsample) features;
// info as ohx_grow_plan_weighted's with info[3] the bin planes of all num_feature features, and info[8] = n_sel
extern "C" __attribute__((visibility("default"))) int ohx_grow_plan_sampled(uint64_t nrow, uint32_t num_feature, float colsample,
                                                                           uint64_t ncuts, int max_depth, int num_cus,
                                                                           uint64_t info[9], uint64_t* levels) {
  try {
    if (max_depth < 1 || max_depth > kGrowMaxDepth) throw OhxError("ohx_grow_plan_sampled: max_depth must be in 1..8");
    const uint32_t n_sel = num_feature <= kGrowMaxFeatures ? grow_num_selected(num_feature, colsample) : 0;
    if (n_sel == 0) throw OhxError("ohx_grow_plan_sampled: 1 to 128 features and a colsample_bytree in (0, 1]");
    write_plan(plan_grow_weighted(nrow, n_sel, ncuts, max_depth, num_cus), (uint64_t)num_feature * nrow, kGrowWeightedPairBytes, info, levels);
    info[8] = n_sel;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// ---- the Deep call (OHXBoosterBoostTreesDeep) ----

// node slots whose histograms a batch of a deep level holds
extern "C" __attribute__((visibility("default"))) uint32_t ohx_grow_deep_batch() { return kGrowDeepBatch; }

// plan_grow_deep.  info and levels as ohx_grow_plan_weighted's, for the min(max_depth, 8) levels kept in LDS; deep: [0]
// batch, [1] blocks of the global histogram kernel, [2] rows such a block takes per trip, [3] bytes of a batch's
// histograms, [4] bytes of a level's candidates, [5] node records of one round
extern "C" __attribute__((visibility("default"))) int ohx_grow_plan_deep(uint64_t nrow, uint32_t num_feature, uint64_t ncuts,
                                                                        int max_depth, int num_cus, uint64_t info[8],
                                                                        uint64_t* levels, uint64_t deep[6]) {
  try {
    if (max_depth < 1 || max_depth > kGrowDeepMaxDepth) throw OhxError("ohx_grow_plan_deep: max_depth must be in 1..18");
    if (nrow == 0) throw OhxError("ohx_grow_plan_deep: no rows");
    const GrowDeepPlan p = plan_grow_deep(nrow, num_feature, ncuts, max_depth, num_cus);
    write_plan(p.lds, (uint64_t)num_feature * nrow, kGrowWeightedPairBytes, info, levels);
    deep[0] = p.batch;
    deep[1] = p.hist_blocks;
    deep[2] = kGrowBlock;
    deep[3] = p.scratch_bytes;
    deep[4] = p.best_bytes;
    deep[5] = p.node_stride;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// plan_grow_deep_sampled over n_sel of the num_feature features (OHXBoosterBoostTreesDeepSampled): info, levels and deep
// as ohx_grow_plan_deep's over n_sel columns, with info[3] the bin planes of all num_feature features
extern "C" __attribute__((visibility("default"))) int ohx_grow_plan_deep_sampled(uint64_t nrow, uint32_t num_feature, uint32_t n_sel,
                                                                                uint64_t ncuts, int max_depth, int num_cus,
                                                                                uint64_t info[8], uint64_t* levels, uint64_t deep[6]) {
  try {
    if (max_depth < 1 || max_depth > kGrowDeepMaxDepth) throw OhxError("ohx_grow_plan_deep_sampled: max_depth must be in 1..18");
    if (nrow == 0) throw OhxError("ohx_grow_plan_deep_sampled: no rows");
    if (num_feature == 0 || num_feature > kGrowMaxFeatures || n_sel == 0 || n_sel > num_feature)
      throw OhxError("ohx_grow_plan_deep_sampled: 1 to 128 features and 1 to num_feature of them selected");
    const GrowDeepPlan p = plan_grow_deep_sampled(nrow, num_feature, n_sel, ncuts, max_depth, num_cus);
    write_plan(p.lds, p.lds.bins_bytes, kGrowWeightedPairBytes, info, levels);
    deep[0] = p.batch;
    deep[1] = p.hist_blocks;
    deep[2] = kGrowBlock;
    deep[3] = p.scratch_bytes;
    deep[4] = p.best_bytes;
    deep[5] = p.node_stride;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// grow_chunked_children: the child ids a block of `width` lanes hands the `count` open nodes of a level whose split
// flags are flag[]; left[s] is written where flag[s] != 0; *splits: their number
extern "C" __attribute__((visibility("default"))) int ohx_grow_deep_children(const uint8_t* flag, uint32_t count, uint32_t width,
                                                                            uint32_t next, uint32_t* left, uint32_t* splits) {
  try {
    if (width == 0) throw OhxError("ohx_grow_deep_children: width must be >= 1");
    *splits = grow_chunked_children(flag, count, width, next, left);
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// ---- the objective's pair (docs/26_objectives.md) ----

// grow.hpp grow_pair over n rows: objective 0 squarederror, 1 pseudohuber with `slope`, 2 quantile with alpha in its place.  w may be NULL (every weight
// 1.0f).  q int64 [n], hq uint32 [n]; *flags: the kGrowFlag* bits the rows raise together (a row that raises one has the
// pair (0, 0)).  An objective or a slope the library refuses is an error.
extern "C" __attribute__((visibility("default"))) int ohx_grow_pairs(uint32_t objective, float slope, const float* pred,
                                                                    const float* y, const float* w, uint64_t n, int64_t* q,
                                                                    uint32_t* hq, uint32_t* flags) {
  try {
    if (objective > kGrowObjQuantile) throw OhxError("ohx_grow_pairs: objective must be 0, 1 or 2");
    if (objective == kGrowObjQuantile && !grow_alpha_sound(slope)) throw OhxError("ohx_grow_pairs: 2^-10 <= alpha <= 1 - 2^-10");
    if (objective == kGrowObjPseudoHuber && !grow_slope_sound(slope)) throw OhxError("ohx_grow_pairs: 2^-10 <= slope <= 256");
    uint32_t raised = 0;
    for (uint64_t r = 0; r < n; ++r) raised |= grow_pair_of(objective, slope, pred[r], y[r], w != nullptr ? w[r] : 1.0f, &q[r], &hq[r]);
    *flags = raised;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// the bytes of the pair planes in the plan of n rows, and the bytes a row
extern "C" __attribute__((visibility("default"))) int ohx_grow_pairs_plan(uint64_t nrow, uint32_t num_feature, uint64_t ncuts,
                                                                         int max_depth, int num_cus, uint64_t info[2]) {
  try {
    if (max_depth < 1 || max_depth > kGrowDeepMaxDepth) throw OhxError("ohx_grow_pairs_plan: max_depth must be in 1..18");
    if (nrow == 0) throw OhxError("ohx_grow_pairs_plan: no rows");
    info[0] = plan_grow_deep(nrow, num_feature, ncuts, max_depth, num_cus).lds.pairs_bytes;
    info[1] = kGrowPairRowBytes;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// ---- reg_alpha, max_delta_step and the metrics (docs/27_regularisation_and_metrics.md) ----

// the header's gain(G, H) of GrowRegHess, as a double
extern "C" __attribute__((visibility("default"))) double ohx_grow_reg_gain(int64_t G, uint64_t H, float lambda, float alpha,
                                                                            float max_delta_step) {
  return GrowRegHess{0.0, alpha, max_delta_step}.gain(G, H, (double)lambda);
}

// out: (leaf, base_weight, sum_hess) of GrowRegHess
extern "C" __attribute__((visibility("default"))) void ohx_grow_reg_leaf(int64_t G, uint64_t H, float eta, float lambda, float alpha,
                                                                         float max_delta_step, float out[3]) {
  const GrowRegHess hess{0.0, alpha, max_delta_step};
  hess.solve_leaf(G, H, eta, lambda, &out[0], &out[1]);
  out[2] = hess.sum_hess(H);
}

// A node's best split over its histograms by GrowRegHess (grow_node_split): out = (valid, key, GL, HL), *loss_chg.
extern "C" __attribute__((visibility("default"))) int ohx_grow_reg_node_split(const int64_t* G, const uint64_t* H, uint32_t num_feature,
                                                                              const uint64_t* cut_ptr, int64_t Gp, uint64_t Hp,
                                                                              float lambda, float min_child_weight, float alpha,
                                                                              float max_delta_step, uint64_t out[4], double* loss_chg) {
  const GrowCand c = grow_node_split(G, H, num_feature, cut_ptr, Gp, Hp, lambda,
                                     GrowRegHess{(double)min_child_weight, alpha, max_delta_step});
  out[0] = c.valid;
  out[1] = c.key;
  out[2] = (uint64_t)c.GL;
  out[3] = c.HL;
  *loss_chg = c.loss_chg;
  return 0;
}

// ---- monotone constraints (docs/28_monotone_constraints.md) ----

// the header's w(G, H; lo, hi) of GrowMonoHess, as a double
extern "C" __attribute__((visibility("default"))) double ohx_grow_mono_weight(int64_t G, uint64_t H, float lambda, float alpha,
                                                                               float max_delta_step, double lo, double hi) {
  return GrowMonoHess{GrowRegHess{0.0, alpha, max_delta_step}, lo, hi, 0}.weight(G, H, (double)lambda);
}

// the header's gain_w(G, H, w), as a double
extern "C" __attribute__((visibility("default"))) double ohx_grow_mono_gain(int64_t G, uint64_t H, float lambda, float alpha, double w) {
  return grow_gain_at((double)G * (1.0 / 16777216.0), grow_hess(H) + (double)lambda, (double)alpha, w);
}

// out: (leaf, base_weight, sum_hess) of GrowMonoHess under the interval (lo, hi)
extern "C" __attribute__((visibility("default"))) void ohx_grow_mono_leaf(int64_t G, uint64_t H, float eta, float lambda, float alpha,
                                                                          float max_delta_step, double lo, double hi, float out[3]) {
  const GrowMonoHess hess{GrowRegHess{0.0, alpha, max_delta_step}, lo, hi, 0};
  hess.solve_leaf(G, H, eta, lambda, &out[0], &out[1]);
  out[2] = hess.sum_hess(H);
}

// A node's best split over its histograms under its interval (lo, hi) and the constraints of the num_feature features
// (grow_mono_node_split): out = (valid, key, GL, HL), *loss_chg, and children = (lo_L, hi_L, lo_R, hi_R).
extern "C" __attribute__((visibility("default"))) int ohx_grow_mono_node_split(const int64_t* G, const uint64_t* H, uint32_t num_feature,
                                                                               const uint64_t* cut_ptr, int64_t Gp, uint64_t Hp,
                                                                               float lambda, float min_child_weight, float alpha,
                                                                               float max_delta_step, double lo, double hi,
                                                                               const int8_t* constraints, uint64_t out[4],
                                                                               double* loss_chg, double children[4]) {
  const GrowCand c = grow_mono_node_split(G, H, num_feature, cut_ptr, Gp, Hp, lambda,
                                          GrowRegHess{(double)min_child_weight, alpha, max_delta_step}, lo, hi, constraints, children);
  out[0] = c.valid;
  out[1] = c.key;
  out[2] = (uint64_t)c.GL;
  out[3] = c.HL;
  *loss_chg = c.loss_chg;
  return 0;
}

// sq of every row by `metric` (0 rmse, 1 mae, 2 pseudohuber with `slope`, 3 quantile with alpha in its place); sound[r] = 0 where the residual is refused
extern "C" __attribute__((visibility("default"))) int ohx_grow_metric_row(uint32_t metric, float slope, const float* pred, const float* y,
                                                                         uint64_t n, uint64_t* sq, uint8_t* sound) {
  try {
    if (metric > kGrowMetricQuantile) throw OhxError("ohx_grow_metric_row: metric must be 0, 1, 2 or 3");
    if (metric == kGrowMetricQuantile && !grow_alpha_sound(slope)) throw OhxError("ohx_grow_metric_row: 2^-10 <= alpha <= 1 - 2^-10");
    if (metric == kGrowMetricPseudoHuber && !grow_slope_sound(slope)) throw OhxError("ohx_grow_metric_row: 2^-10 <= slope <= 256");
    for (uint64_t r = 0; r < n; ++r) sound[r] = grow_metric_row_of(metric, slope, pred[r], y[r], &sq[r]) ? 1 : 0;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// s: (p2, p1, p0); W: the sum of hq
extern "C" __attribute__((visibility("default"))) double ohx_grow_weighted_mean(const uint64_t s[3], uint64_t W) {
  GrowWideSum x;
  x.p2 = s[0];
  x.p1 = s[1];
  x.p0 = s[2];
  return grow_wide_mean(x, W);
}

// ---- the quantile objective (docs/32_quantile_objective.md) ----

// s: (p2, p1, p0); W: the sum of hq
extern "C" __attribute__((visibility("default"))) double ohx_grow_weighted_quantile(const uint64_t s[3], uint64_t W) {
  GrowWideSum x;
  x.p2 = s[0];
  x.p1 = s[1];
  x.p0 = s[2];
  return grow_wide_quantile(x, W);
}

// grow_quantile.hpp grow_quantile_pick on one leaf's bins of pass `pass`; st = (prefix, below, W) in and out.  Returns 1
// where a digit was picked, 0 where the leaf holds no weight.
extern "C" __attribute__((visibility("default"))) int ohx_grow_quantile_pick(const uint64_t bins[256], uint32_t pass, float alpha,
                                                                            uint64_t st[3]) {
  GrowQuantileLeaf leaf;
  leaf.prefix = (uint32_t)st[0];
  leaf.below = st[1];
  leaf.W = st[2];
  const bool found = pass < kGrowQuantilePasses && grow_alpha_sound(alpha) && grow_quantile_pick(bins, pass, grow_alpha_q(alpha), &leaf);
  st[0] = leaf.prefix;
  st[1] = leaf.below;
  st[2] = leaf.W;
  return found ? 1 : 0;
}

// grow_quantile.hpp plan_grow_quantile over the row_blocks of plan_grow_weighted, which does not depend on the columns: the
// grid launch_grow_tree_quantile gives grow_quantile_pass_kernel.  info: [0] blocks of the pass kernel over the rows
// (gridDim.x), [1] rows such a block takes per trip, [2] leaves a block holds, [3] leaf groups (gridDim.y), [4] row_blocks
extern "C" __attribute__((visibility("default"))) int ohx_grow_quantile_plan(uint64_t nrow, int max_depth, int num_cus, uint64_t info[5]) {
  try {
    if (max_depth < 1 || max_depth > kGrowMaxDepth) throw OhxError("ohx_grow_quantile_plan: max_depth must be in 1..8");
    if (nrow == 0) throw OhxError("ohx_grow_quantile_plan: no rows");
    const uint32_t row_blocks = plan_grow_weighted(nrow, 1, 0, max_depth, num_cus).row_blocks;
    const GrowQuantilePlan p = plan_grow_quantile(nrow, max_depth, row_blocks);
    info[0] = p.blocks;
    info[1] = kGrowHistBlock;
    info[2] = p.group;
    info[3] = p.groups;
    info[4] = row_blocks;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// The whole select as the device runs it, with host counting: rows at node pos[r] with hessian hq[r] (0: the row does
// not count) and residual y[r] - pred[r]; leaves[s] is the node of slot s.  Four passes of bins[slot][digit] over the rows
// whose key carries their leaf's prefix, each followed by the picks.  found[s] = 0 where slot s holds no weight; else
// key[s] = k*, value[s] = float(cuts_unkey(k*)) * eta and W[s] the leaf's weight.
extern "C" __attribute__((visibility("default"))) int ohx_grow_quantile_leaves(const uint16_t* pos, const uint32_t* hq, const float* pred,
                                                                              const float* y, uint64_t n, const uint16_t* leaves,
                                                                              uint32_t nleaves, float alpha, float eta, uint8_t* found,
                                                                              uint32_t* key, float* value, uint64_t* W) {
  try {
    if (nleaves > kGrowQuantileMaxLeaves) throw OhxError("ohx_grow_quantile_leaves: at most 256 leaves");
    if (!grow_alpha_sound(alpha)) throw OhxError("ohx_grow_quantile_leaves: 2^-10 <= alpha <= 1 - 2^-10");
    std::vector<uint16_t> slot_of(kGrowMaxNodes, (uint16_t)kGrowQuantileNoSlot);
    for (uint32_t s = 0; s < nleaves; ++s) {
      if (leaves[s] >= kGrowMaxNodes || slot_of[leaves[s]] != kGrowQuantileNoSlot) throw OhxError("ohx_grow_quantile_leaves: a leaf's node id");
      slot_of[leaves[s]] = (uint16_t)s;
    }
    const uint32_t alpha_q = grow_alpha_q(alpha);
    std::vector<GrowQuantileLeaf> leaf(nleaves);
    std::vector<uint8_t> live(nleaves, 1);
    std::vector<uint64_t> bins((size_t)nleaves * kGrowQuantileDigits);
    for (uint32_t pass = 0; pass < kGrowQuantilePasses; ++pass) {
      std::fill(bins.begin(), bins.end(), 0);
      for (uint64_t r = 0; r < n; ++r) {
        if (hq[r] == 0 || pos[r] >= kGrowMaxNodes) continue;
        const uint32_t s = slot_of[pos[r]];
        if (s >= nleaves) continue;
        const uint32_t k = grow_quantile_key(pred[r], y[r]);
        if (!grow_quantile_matches(k, leaf[s].prefix, pass)) continue;
        bins[(size_t)s * kGrowQuantileDigits + grow_quantile_digit(k, pass)] += hq[r];
      }
      for (uint32_t s = 0; s < nleaves; ++s)
        if (live[s]) live[s] = grow_quantile_pick(bins.data() + (size_t)s * kGrowQuantileDigits, pass, alpha_q, &leaf[s]) ? 1 : 0;
    }
    for (uint32_t s = 0; s < nleaves; ++s) {
      found[s] = live[s];
      key[s] = live[s] ? leaf[s].prefix : 0;
      value[s] = live[s] ? grow_quantile_value(leaf[s].prefix, eta) : 0.0f;
      W[s] = leaf[s].W;
    }
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}
