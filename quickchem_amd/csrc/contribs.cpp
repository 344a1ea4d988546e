// Host preparation of per-feature contributions (contribs.hpp).  Host logic only: the arithmetic a row's
// contributions need happens in contribs.hip.
#include "contribs.hpp"

#include <algorithm>
#include <cmath>

namespace ohx {

void check_contrib_cover(const Forest& f) {
  for (size_t ti = 0; ti < f.trees.size(); ++ti) {
    const Tree& t = f.trees[ti];
    std::vector<int32_t> stack{0};
    while (!stack.empty()) {
      const size_t n = (size_t)stack.back();
      stack.pop_back();
      if (t.is_leaf(n)) continue;
      const float c = t.sum_hess[n];
      if (!std::isfinite(c) || !(c > 0.0f))
        throw OhxError("the model has no cover statistics (tree " + std::to_string(ti) + ", node " + std::to_string(n) +
                       ": sum_hess " + std::to_string(c) + "); feature contributions need a cover > 0 at every split");
      stack.push_back(t.left[n]);
      stack.push_back(t.right[n]);
    }
  }
}

namespace {

float fill_means(const Tree& t, int32_t n, std::vector<float>* means) {
  float result;
  if (t.is_leaf((size_t)n)) {
    result = t.value[(size_t)n];
  } else {
    const int32_t l = t.left[(size_t)n], r = t.right[(size_t)n];
    result = fill_means(t, l, means) * t.sum_hess[(size_t)l];
    result += fill_means(t, r, means) * t.sum_hess[(size_t)r];
    result /= t.sum_hess[(size_t)n];
  }
  (*means)[(size_t)n] = result;
  return result;
}

struct PathBuilder {
  const Tree& t;
  std::vector<PathElem> path;                     // distinct features from the root down to the current node
  std::vector<std::pair<std::vector<PathElem>, float>> leaves;

  void walk(int32_t n) {
    if (t.is_leaf((size_t)n)) {
      if (path.size() > (size_t)kMaxPathLen)
        throw OhxError("a root-to-leaf path splits on " + std::to_string(path.size()) +
                       " distinct features; feature contributions support at most " + std::to_string(kMaxPathLen));
      if (!path.empty()) leaves.emplace_back(path, t.value[(size_t)n]);
      return;
    }
    const uint32_t feat = t.feature[(size_t)n];
    const float cond = t.value[(size_t)n];
    const float cover = t.sum_hess[(size_t)n];
    for (int side = 0; side < 2; ++side) {
      const int32_t c = side == 0 ? t.left[(size_t)n] : t.right[(size_t)n];
      const uint32_t miss = (t.default_left[(size_t)n] != 0) == (side == 0) ? 1u : 0u;
      const float z = t.sum_hess[(size_t)c] / cover;
      const size_t saved = path.size();
      size_t k = 0;
      while (k < path.size() && (path[k].feat & 0x7FFFFFFFu) != feat) ++k;
      PathElem before{};
      if (k == path.size()) path.push_back(PathElem{feat | 0x80000000u, NAN, NAN, 1.0f});
      else before = path[k];
      PathElem& e = path[k];
      if (side == 0) e.hi = std::isnan(e.hi) ? cond : std::min(e.hi, cond);    // x < cond
      else e.lo = std::isnan(e.lo) ? cond : std::max(e.lo, cond);              // x >= cond
      if (!miss) e.feat &= 0x7FFFFFFFu;
      e.z *= z;
      walk(c);
      if (path.size() > saved) path.pop_back();
      else path[k] = before;
    }
  }
};

}  // namespace

std::vector<float> node_means(const Tree& t) {
  std::vector<float> means(t.size(), 0.0f);
  fill_means(t, 0, &means);
  return means;
}

float contrib_bias(const Forest& f, const std::vector<std::vector<float>>& means, uint32_t t0, uint32_t t1,
                   float margin_base) {
  (void)f;
  float bias = 0.0f;
  for (uint32_t t = t0; t < t1; ++t) bias += means[t][0];
  bias += margin_base;
  return bias;
}

std::vector<ContribNode> emit_contrib_nodes(const Forest& f, const std::vector<std::vector<float>>& means,
                                            std::vector<uint32_t>* roots) {
  std::vector<ContribNode> out;
  roots->clear();
  for (size_t ti = 0; ti < f.trees.size(); ++ti) {
    const Tree& t = f.trees[ti];
    const uint32_t base = (uint32_t)out.size();
    if ((uint64_t)base + t.size() >= 0xFFFFFFF0ull) throw OhxError("booster too large: more than 2**32 nodes");
    roots->push_back(base);
    for (size_t i = 0; i < t.size(); ++i) {
      ContribNode nd;
      nd.value = t.value[i];
      nd.left = t.is_leaf(i) ? 0u : base + (uint32_t)t.left[i];
      nd.feat_dl = t.is_leaf(i) ? 0u : (t.feature[i] | ((uint32_t)(t.default_left[i] != 0) << 31));
      nd.mean = means[ti][i];
      out.push_back(nd);
    }
  }
  return out;
}

std::vector<float> unwind_coefficients() {
  std::vector<float> c((size_t)kCoefStride * kCoefStride * 4, 0.0f);
  for (int d = 1; d <= kMaxPathLen; ++d)
    for (int i = 0; i < d; ++i) {
      float* q = &c[((size_t)d * kCoefStride + (size_t)i) * 4];
      q[0] = (float)((double)(d + 1) / (double)(i + 1));
      q[1] = (float)((double)(d - i) / (double)(d + 1));
      q[2] = (float)((double)(d + 1) / (double)(d - i));
    }
  return c;
}

int path_class(uint32_t len) {
  for (int c = 0; c < kPathClasses; ++c)
    if (len <= (uint32_t)kPathClassMax[c]) return c;
  return kPathClasses - 1;
}

PathTable build_path_table(const Forest& f) {
  PathTable pt;
  pt.class_start.reserve(f.trees.size() * (kPathClasses + 1));
  for (const Tree& t : f.trees) {
    PathBuilder pb{t, {}, {}};
    pb.walk(0);
    // length classes in order; inside a class the paths keep the depth-first order they were found in
    std::vector<uint32_t> order(pb.leaves.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      return path_class((uint32_t)pb.leaves[a].first.size()) < path_class((uint32_t)pb.leaves[b].first.size());
    });
    int cls = 0;
    for (uint32_t i : order) {
      const uint32_t len = (uint32_t)pb.leaves[i].first.size();
      while (cls <= path_class(len)) {
        pt.class_start.push_back((uint32_t)pt.heads.size());
        ++cls;
      }
      if (pt.elems.size() + len >= 0xFFFFFFF0ull) throw OhxError("booster too large: more than 2**32 path elements");
      pt.heads.push_back(PathHead{(uint32_t)pt.elems.size(), len, pb.leaves[i].second, 0u});
      pt.elems.insert(pt.elems.end(), pb.leaves[i].first.begin(), pb.leaves[i].first.end());
      pt.sum_sq += (uint64_t)(len + 1) * (len + 1);
      pt.max_len = std::max(pt.max_len, len);
    }
    while (cls <= kPathClasses) {
      pt.class_start.push_back((uint32_t)pt.heads.size());
      ++cls;
    }
  }
  return pt;
}

// The split rule of both explanation launches.  `units` = the direct shape's waves; a batch whose direct waves leave
// most of the chip's wave slots empty has its trees split over as many tree groups as fill them, each wave keeping
// nfeat x 64 floats of `part` per tree.
static ContribsPlan plan_split(uint64_t units, uint32_t nfeat, uint32_t ntree, bool allow_split) {
  ContribsPlan p;
  if (!allow_split || units == 0 || ntree < 2 || units * 2 > kWaveSlots) return p;
  const uint64_t part = units * ntree * (uint64_t)nfeat * kContribsTileRows;
  if (part * sizeof(float) > kPartBudgetBytes) return p;
  uint64_t want = (kWaveSlots + units - 1) / units;   // tree groups that fill the chip's wave slots
  if (want > ntree) want = ntree;
  if (want < 2) return p;
  p.trees_per_group = (uint32_t)((ntree + want - 1) / want);
  p.groups = (ntree + p.trees_per_group - 1) / p.trees_per_group;
  p.split = p.groups > 1;
  p.part_floats = p.split ? part : 0;
  return p;
}

static uint64_t tiles_of(uint64_t nrow) { return (nrow + kContribsTileRows - 1) / kContribsTileRows; }

// contributions: one direct wave per tile
ContribsPlan plan_contribs(uint64_t nrow, uint32_t nfeat, uint32_t ntree, bool allow_split) {
  return plan_split(tiles_of(nrow), nfeat, ntree, allow_split);
}

FeaturePathIndex build_feature_path_index(const PathTable& pt, uint32_t ntree, uint32_t nfeat) {
  constexpr int K = kPathClasses;
  FeaturePathIndex ix;
  ix.start.assign((size_t)ntree * nfeat * (K + 1), 0u);
  std::vector<uint32_t> count((size_t)ntree * nfeat * K, 0u);
  for (uint32_t t = 0; t < ntree; ++t)
    for (int c = 0; c < K; ++c)
      for (uint32_t p = pt.class_start[(size_t)t * (K + 1) + c]; p < pt.class_start[(size_t)t * (K + 1) + c + 1]; ++p)
        for (uint32_t k = 0; k < pt.heads[p].len; ++k)
          ++count[((size_t)t * nfeat + (pt.elems[pt.heads[p].first + k].feat & 0x7FFFFFFFu)) * K + c];
  uint32_t at = 0;
  for (size_t tf = 0; tf < (size_t)ntree * nfeat; ++tf) {
    for (int c = 0; c < K; ++c) {
      ix.start[tf * (K + 1) + c] = at;
      at += count[tf * K + c];
    }
    ix.start[tf * (K + 1) + K] = at;
  }
  ix.paths.resize(at);
  std::vector<uint32_t> cursor(count.size());
  for (size_t tf = 0; tf < (size_t)ntree * nfeat; ++tf)
    for (int c = 0; c < K; ++c) cursor[tf * K + c] = ix.start[tf * (K + 1) + c];
  for (uint32_t t = 0; t < ntree; ++t)
    for (int c = 0; c < K; ++c)
      for (uint32_t p = pt.class_start[(size_t)t * (K + 1) + c]; p < pt.class_start[(size_t)t * (K + 1) + c + 1]; ++p)
        for (uint32_t k = 0; k < pt.heads[p].len; ++k)
          ix.paths[cursor[((size_t)t * nfeat + (pt.elems[pt.heads[p].first + k].feat & 0x7FFFFFFFu)) * K + c]++] = p;
  return ix;
}

// interactions: one direct wave per (tile, conditioning feature)
ContribsPlan plan_interactions(uint64_t nrow, uint32_t nfeat, uint32_t ntree, bool allow_split) {
  return plan_split(tiles_of(nrow) * nfeat, nfeat, ntree, allow_split);
}

}  // namespace ohx
