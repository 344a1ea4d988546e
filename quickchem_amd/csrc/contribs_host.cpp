// Test support (libohx_synth.so), not a prediction path: a CPU restatement of per-feature contributions following
// xgboost 1.6.0's recursive RegTree::TreeShap (exact) and CalculateContributionsApprox in float, threaded over rows,
// and of its PredictInteractionContributions (TreeShap's condition / condition_feature, ohx_interactions_cpu).
// The GPU kernels (contribs.hip) are checked against it: approximate mode bit for bit (same node means, same order of
// additions), exact mode to rounding (the kernels evaluate the same recurrences per leaf path).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "contribs.hpp"
#include "forest.hpp"

using namespace ohx;

namespace ohx {
void synth_set_error(const std::string& m);   // synth_host.cpp
}

namespace {

struct Elem {
  int feature;
  float zero_fraction, one_fraction, pweight;
};

void extend_path(Elem* path, unsigned depth, float zero_fraction, float one_fraction, int feature) {
  path[depth].feature = feature;
  path[depth].zero_fraction = zero_fraction;
  path[depth].one_fraction = one_fraction;
  path[depth].pweight = depth == 0 ? 1.0f : 0.0f;
  for (int i = (int)depth - 1; i >= 0; --i) {
    path[i + 1].pweight += one_fraction * path[i].pweight * (float)(i + 1) / (float)(depth + 1);
    path[i].pweight = zero_fraction * path[i].pweight * (float)(depth - i) / (float)(depth + 1);
  }
}

void unwind_path(Elem* path, unsigned depth, unsigned index) {
  const float one_fraction = path[index].one_fraction;
  const float zero_fraction = path[index].zero_fraction;
  float next_one_portion = path[depth].pweight;
  for (int i = (int)depth - 1; i >= 0; --i) {
    if (one_fraction != 0) {
      const float tmp = path[i].pweight;
      path[i].pweight = next_one_portion * (float)(depth + 1) / ((float)(i + 1) * one_fraction);
      next_one_portion = tmp - path[i].pweight * zero_fraction * (float)(depth - i) / (float)(depth + 1);
    } else {
      path[i].pweight = (path[i].pweight * (float)(depth + 1)) / (zero_fraction * (float)(depth - i));
    }
  }
  for (unsigned i = index; i < depth; ++i) {
    path[i].feature = path[i + 1].feature;
    path[i].zero_fraction = path[i + 1].zero_fraction;
    path[i].one_fraction = path[i + 1].one_fraction;
  }
}

float unwound_path_sum(const Elem* path, unsigned depth, unsigned index) {
  const float one_fraction = path[index].one_fraction;
  const float zero_fraction = path[index].zero_fraction;
  float next_one_portion = path[depth].pweight;
  float total = 0;
  for (int i = (int)depth - 1; i >= 0; --i) {
    if (one_fraction != 0) {
      const float tmp = next_one_portion * (float)(depth + 1) / ((float)(i + 1) * one_fraction);
      total += tmp;
      next_one_portion = path[i].pweight - tmp * zero_fraction * ((float)(depth - i) / (float)(depth + 1));
    } else if (zero_fraction != 0) {
      total += (path[i].pweight / zero_fraction) / ((float)(depth - i) / (float)(depth + 1));
    }
  }
  return total;
}

struct Row {
  const float* x;
  uint64_t ncol;
  float missing;
  bool missing_is_nan;
  bool is_missing(uint32_t f) const {
    if (f >= ncol) return true;
    const float v = x[f];
    return v != v || (!missing_is_nan && v == missing);
  }
  int32_t next(const Tree& t, int32_t n) const {
    const uint32_t f = t.feature[(size_t)n];
    if (is_missing(f)) return t.default_left[(size_t)n] ? t.left[(size_t)n] : t.right[(size_t)n];
    return x[f] < t.value[(size_t)n] ? t.left[(size_t)n] : t.right[(size_t)n];
  }
};

// condition 0: plain TreeSHAP.  condition +1 / -1: feature condition_feature is "on" / "off" - it never enters the
// path; a split on it sends the whole weight down the hot child (on), or scales each child's by its zero fraction
// (off), through condition_fraction (1.6.0).
void tree_shap(const Tree& t, const Row& row, float* phi, int32_t n, unsigned depth, Elem* parent_path,
               float parent_zero, float parent_one, int parent_feature, int condition = 0,
               unsigned condition_feature = 0, float condition_fraction = 1) {
  if (condition_fraction == 0) return;
  Elem* path = parent_path + depth + 1;
  std::copy(parent_path, parent_path + depth + 1, path);
  if (condition == 0 || condition_feature != (unsigned)parent_feature)
    extend_path(path, depth, parent_zero, parent_one, parent_feature);
  if (t.is_leaf((size_t)n)) {
    for (unsigned i = 1; i <= depth; ++i) {
      const float w = unwound_path_sum(path, depth, i);
      const Elem& el = path[i];
      phi[el.feature] += w * (el.one_fraction - el.zero_fraction) * t.value[(size_t)n] * condition_fraction;
    }
    return;
  }
  const uint32_t split = t.feature[(size_t)n];
  const int32_t hot = row.next(t, n);
  const int32_t cold = hot == t.left[(size_t)n] ? t.right[(size_t)n] : t.left[(size_t)n];
  const float w = t.sum_hess[(size_t)n];
  const float hot_zero = t.sum_hess[(size_t)hot] / w;
  const float cold_zero = t.sum_hess[(size_t)cold] / w;
  float incoming_zero = 1, incoming_one = 1;
  unsigned k = 0;
  for (; k <= depth; ++k)
    if (path[k].feature == (int)split) break;
  if (k != depth + 1) {
    incoming_zero = path[k].zero_fraction;
    incoming_one = path[k].one_fraction;
    unwind_path(path, depth, k);
    depth -= 1;
  }
  float hot_condition = condition_fraction, cold_condition = condition_fraction;
  if (condition > 0 && split == condition_feature) {
    cold_condition = 0;
    depth -= 1;
  } else if (condition < 0 && split == condition_feature) {
    hot_condition *= hot_zero;
    cold_condition *= cold_zero;
    depth -= 1;
  }
  tree_shap(t, row, phi, hot, depth + 1, path, hot_zero * incoming_zero, incoming_one, (int)split, condition,
            condition_feature, hot_condition);
  tree_shap(t, row, phi, cold, depth + 1, path, cold_zero * incoming_zero, 0, (int)split, condition,
            condition_feature, cold_condition);
}

void tree_approx(const Tree& t, const std::vector<float>& means, const Row& row, float* out) {
  float node_value = means[0];
  if (t.is_leaf(0)) return;
  int32_t n = 0;
  uint32_t split = 0;
  while (!t.is_leaf((size_t)n)) {
    split = t.feature[(size_t)n];
    n = row.next(t, n);
    const float v = means[(size_t)n];
    out[split] += v - node_value;
    node_value = v;
  }
  out[split] += t.value[(size_t)n] - node_value;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int ohx_contribs_cpu(const void* model, uint64_t len, const float* rows,
                                                                      uint64_t nrow, uint64_t ncol, float missing,
                                                                      int approximate, unsigned ntree_limit, float* out) {
  try {
    Forest f = load_model_buffer(model, (size_t)len);
    f.validate();
    check_contrib_cover(f);
    const float base = f.margin_base();
    const uint32_t F = f.num_feature;
    if (ncol > F) throw OhxError("more columns than the booster has features");
    const uint32_t T = (uint32_t)f.trees.size();
    const uint32_t t1 = (ntree_limit == 0 || ntree_limit > T) ? T : ntree_limit;
    std::vector<std::vector<float>> means;
    int max_depth = 0;
    for (const Tree& t : f.trees) means.push_back(node_means(t));
    max_depth = f.max_depth();
    const float bias = contrib_bias(f, means, 0, t1, base);
    const size_t path_len = (size_t)(max_depth + 2) * (max_depth + 3) / 2 + 2;
#pragma omp parallel
    {
      std::vector<Elem> path(path_len);
      std::vector<float> tree(F + 1);
#pragma omp for schedule(dynamic, 64)
      for (int64_t r = 0; r < (int64_t)nrow; ++r) {
        const Row row{rows + (size_t)r * ncol, ncol, missing, missing != missing};
        float* o = out + (size_t)r * (F + 1);
        for (uint32_t j = 0; j <= F; ++j) o[j] = 0.0f;
        for (uint32_t t = 0; t < t1; ++t) {
          std::fill(tree.begin(), tree.end(), 0.0f);
          if (approximate) tree_approx(f.trees[t], means[t], row, tree.data());
          else tree_shap(f.trees[t], row, tree.data(), 0, 0, path.data(), 1, 1, -1);
          for (uint32_t j = 0; j < F; ++j) o[j] += tree[j];
        }
        o[F] = bias;
      }
    }
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// 1.6.0's PredictInteractionContributions: out is [nrow][F + 1][F + 1].  Per row the plain contributions (the
// diagonal's), then for each i = 0 .. F the passes conditioned on i off and on - each a whole 1.6.0 PredictContribution
// (tree by tree into the row, its bias column the margin base alone when conditioned); off-diagonals
// (on - off) / 2.0 as 1.6.0 writes it, then the diagonal from 0 in its order.
extern "C" __attribute__((visibility("default"))) int ohx_interactions_cpu(const void* model, uint64_t len,
                                                                          const float* rows, uint64_t nrow,
                                                                          uint64_t ncol, float missing, int approximate,
                                                                          unsigned ntree_limit, float* out) {
  try {
    Forest f = load_model_buffer(model, (size_t)len);
    f.validate();
    check_contrib_cover(f);
    const float base = f.margin_base();
    const uint32_t F = f.num_feature;
    if (ncol > F) throw OhxError("more columns than the booster has features");
    const uint32_t T = (uint32_t)f.trees.size();
    const uint32_t t1 = (ntree_limit == 0 || ntree_limit > T) ? T : ntree_limit;
    std::vector<std::vector<float>> means;
    for (const Tree& t : f.trees) means.push_back(node_means(t));
    const int max_depth = f.max_depth();
    const float bias = contrib_bias(f, means, 0, t1, base);
    const size_t path_len = (size_t)(max_depth + 2) * (max_depth + 3) / 2 + 2;
    const size_t F1 = (size_t)F + 1;
    std::vector<float> diags(nrow * F1);
#pragma omp parallel
    {
      std::vector<Elem> path(path_len);
      std::vector<float> tree(F1), on(F1), off(F1);
      auto contribution = [&](const Row& row, int condition, unsigned feature, float* o) {
        for (uint32_t j = 0; j <= F; ++j) o[j] = 0.0f;
        for (uint32_t t = 0; t < t1; ++t) {
          std::fill(tree.begin(), tree.end(), 0.0f);
          if (approximate) tree_approx(f.trees[t], means[t], row, tree.data());
          else tree_shap(f.trees[t], row, tree.data(), 0, 0, path.data(), 1, 1, -1, condition, feature, 1);
          for (uint32_t j = 0; j < F; ++j) o[j] += tree[j];
        }
        o[F] = condition == 0 ? bias : base;
      };
      // the plain pass of every row first, then every (row, i) on its own: a row's 2F + 3 passes spread over threads
#pragma omp for schedule(dynamic, 1)
      for (int64_t r = 0; r < (int64_t)nrow; ++r) {
        const Row row{rows + (size_t)r * ncol, ncol, missing, missing != missing};
        contribution(row, 0, 0, &diags[(size_t)r * F1]);
      }
#pragma omp for schedule(dynamic, 1)
      for (int64_t ri = 0; ri < (int64_t)(nrow * F1); ++ri) {
        const size_t r = (size_t)ri / F1, i = (size_t)ri % F1;
        const Row row{rows + r * ncol, ncol, missing, missing != missing};
        const float* diag = &diags[r * F1];
        contribution(row, -1, (unsigned)i, off.data());
        contribution(row, 1, (unsigned)i, on.data());
        float* o = out + r * F1 * F1 + i * F1;
        o[i] = 0;
        for (size_t k = 0; k < F1; ++k) {
          if (k == i) {
            o[i] += diag[k];
          } else {
            o[k] = (on[k] - off[k]) / 2.0;
            o[i] -= o[k];
          }
        }
      }
    }
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// Sizes of exact interactions' feature-path index and the path sums its cost follows: stats[0] index bytes,
// [1] paths, [2] sum d, [3] sum d^2, [4] sum d^3 (d = a path's distinct features).
extern "C" __attribute__((visibility("default"))) int ohx_interactions_table_stats(const void* model, uint64_t len,
                                                                                  uint64_t* stats) {
  try {
    Forest f = load_model_buffer(model, (size_t)len);
    f.validate();
    check_contrib_cover(f);
    const PathTable pt = build_path_table(f);
    stats[0] = build_feature_path_index(pt, (uint32_t)f.trees.size(), f.num_feature).bytes();
    stats[1] = pt.heads.size();
    stats[2] = stats[3] = stats[4] = 0;
    for (const PathHead& h : pt.heads) {
      const uint64_t d = h.len;
      stats[2] += d;
      stats[3] += d * d;
      stats[4] += d * d * d;
    }
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// The launch shape of exact interactions (contribs.cpp plan_interactions): plan[0] split (0 / 1), [1] tree groups,
// [2] trees per group, [3] direct launches (0 when split), [4] the part floats a split asks for.
extern "C" __attribute__((visibility("default"))) int ohx_interactions_plan(uint64_t nrow, uint32_t nfeat,
                                                                           uint32_t ntree, int allow_split,
                                                                           uint64_t* plan) {
  const ContribsPlan p = plan_interactions(nrow, nfeat, ntree, allow_split != 0);
  const uint64_t tiles = (nrow + kContribsTileRows - 1) / kContribsTileRows;
  const uint64_t per = interactions_tiles_per_launch(nfeat);
  plan[0] = p.split ? 1 : 0;
  plan[1] = p.groups;
  plan[2] = p.trees_per_group;
  plan[3] = p.split ? 0 : (tiles + per - 1) / per;
  plan[4] = p.part_floats;
  return 0;
}

// Sizes of the exact mode's path table for a model, as the library builds it: stats[0] bytes, [1] paths,
// [2] elements, [3] sum over paths of (len + 1)^2, [4] longest path (distinct features).
extern "C" __attribute__((visibility("default"))) int ohx_contribs_table_stats(const void* model, uint64_t len,
                                                                              uint64_t* stats) {
  try {
    Forest f = load_model_buffer(model, (size_t)len);
    f.validate();
    check_contrib_cover(f);
    const PathTable pt = build_path_table(f);
    stats[0] = pt.bytes();
    stats[1] = pt.heads.size();
    stats[2] = pt.elems.size();
    stats[3] = pt.sum_sq;
    stats[4] = pt.max_len;
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// The launch shape the library picks for a batch (contribs.cpp plan_contribs): plan[0] split (0 / 1), [1] tree groups,
// [2] trees per group, [3] direct launches of exact mode (0 when split; approximate mode launches once below 2**24
// tiles).
extern "C" __attribute__((visibility("default"))) int ohx_contribs_plan(uint64_t nrow, uint32_t nfeat, uint32_t ntree,
                                                                       int allow_split, uint64_t* plan) {
  const ContribsPlan p = plan_contribs(nrow, nfeat, ntree, allow_split != 0);
  const uint64_t tiles = (nrow + kContribsTileRows - 1) / kContribsTileRows;
  plan[0] = p.split ? 1 : 0;
  plan[1] = p.groups;
  plan[2] = p.trees_per_group;
  plan[3] = p.split ? 0 : (tiles + kDirectTilesPerLaunch - 1) / kDirectTilesPerLaunch;
  return 0;
}
