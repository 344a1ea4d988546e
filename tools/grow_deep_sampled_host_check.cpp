// The plan of row and column subsampling for trees deeper than eight levels (csrc/grow.hpp plan_grow_deep_sampled,
// grow.cpp) in a program of its own, for a build with -fsanitize=address,undefined (CPU only;
// tests/test_grow_deep_sampled_cpu.py builds and runs it): the plan over its edges - 1 to 2^31 rows, 1 to 128 features,
// every n_sel from 1 to F and every depth from 1 to 18 - against plan_grow_weighted, plan_grow_deep and the formulas of
// the header.  Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_deep_sampled_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "grow.hpp"

using namespace ohx;

static long failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      ++failures;                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);            \
    }                                                            \
  } while (0)

static bool same_levels(const GrowPlan& a, const GrowPlan& b) {
  if (a.levels.size() != b.levels.size() || a.row_blocks != b.row_blocks || a.bin_lds_bytes != b.bin_lds_bytes ||
      a.hist_bytes != b.hist_bytes)
    return false;
  for (size_t d = 0; d < a.levels.size(); ++d) {
    const GrowLevelPlan &x = a.levels[d], &y = b.levels[d];
    if (x.slots != y.slots || x.node_group != y.node_group || x.feat_group != y.feat_group || x.node_groups != y.node_groups ||
        x.feat_groups != y.feat_groups || x.hist_blocks != y.hist_blocks || x.lds_bytes != y.lds_bytes)
      return false;
  }
  return true;
}

static long plans = 0;

static void check_plan(uint64_t n, uint32_t F, uint32_t n_sel, int depth, int cus) {
  ++plans;
  const uint64_t ncuts = (uint64_t)F * kGrowMaxCuts;
  const GrowDeepPlan p = plan_grow_deep_sampled(n, F, n_sel, ncuts, depth, cus);
  const int top = std::min(depth, kGrowMaxDepth);
  // levels 0 - 7: the weighted plan over n_sel columns, with the bin planes of every feature
  GrowPlan w = plan_grow_weighted(n, n_sel, ncuts, top, cus);
  EXPECT(p.lds.levels.size() == (size_t)top && same_levels(p.lds, w));
  EXPECT(p.lds.bins_bytes == (uint64_t)F * n);
  // the deep levels: compact histograms of a batch, the candidates of a level, the stride
  const uint64_t open = std::max<uint64_t>(1, std::min<uint64_t>(1ull << (depth - 1), n));
  EXPECT(grow_deep_max_open(n, depth) == open);
  EXPECT(p.batch == kGrowDeepBatch && p.hist_blocks == w.row_blocks && p.hist_blocks >= 1);
  EXPECT((uint64_t)(p.hist_blocks - 1) * kGrowBlock < n);
  EXPECT(p.scratch_bytes == (depth > kGrowMaxDepth ? std::min<uint64_t>(kGrowDeepBatch, open) * n_sel * kGrowBins * 16 : 0));
  EXPECT(p.best_bytes == std::max<uint64_t>(open, 1ull << (top - 1)) * n_sel * sizeof(GrowCand));
  EXPECT(p.node_stride == std::min<uint64_t>(1ull << (depth + 1), 2 * n) && p.node_stride == grow_deep_node_stride(n, depth));
  // every level's candidates fit `best`, and every batch's histograms the scratch
  EXPECT(p.best_bytes >= (uint64_t)(1u << (top - 1)) * n_sel * sizeof(GrowCand));
  EXPECT(p.scratch_bytes <= (uint64_t)kGrowDeepBatch * F * kGrowBins * 16);
  if (n_sel == F) {   // every feature: plan_grow_deep itself
    const GrowDeepPlan q = plan_grow_deep(n, F, ncuts, depth, cus);
    EXPECT(same_levels(p.lds, q.lds) && p.lds.bins_bytes == q.lds.bins_bytes && p.batch == q.batch && p.hist_blocks == q.hist_blocks &&
           p.scratch_bytes == q.scratch_bytes && p.best_bytes == q.best_bytes && p.node_stride == q.node_stride);
  }
}

int main() {
  const uint64_t rows[] = {1, 2, 63, 64, 65, 255, 256, 257, 4097, 1ull << 20, 55987200ull, (1ull << 31) - 1, 1ull << 31};
  const uint32_t feats[] = {1, 2, 3, 27, 41, 127, 128};
  for (uint64_t n : rows)
    for (uint32_t F : feats)
      for (uint32_t n_sel = 1; n_sel <= F; ++n_sel)
        for (int depth = 1; depth <= kGrowDeepMaxDepth; ++depth) check_plan(n, F, n_sel, depth, n % 2 ? 256 : 1);
  // a device that reports no compute unit plans as one
  check_plan(4097, 27, 13, 18, 0);
  check_plan(4097, 27, 13, 18, -5);
  printf("grow_deep_sampled_host_check: %ld plans, %ld failures\n", plans, failures);
  return failures == 0 ? 0 : 1;
}
