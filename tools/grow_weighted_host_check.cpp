// The host functions of boosting with row weights (csrc/grow.hpp, grow.cpp) in a program of their own, for a build with
// -fsanitize=address,undefined (CPU only; tests/test_grow_weighted_cpu.py builds and runs it): the 40-pair launch plan
// from 1 to 2^31 rows and 1 to 128 features, the (S, W) conversion and the comparison at the accumulators' limits, and
// the weighted split choice and leaf solve on histograms with sums as large as 2^31 rows of the largest weight and
// gradient make them.  Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_weighted_host_check <histograms> <seed>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
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

static void check_plans() {
  const uint64_t rows[] = {1, 63, 1024, 1025, 4097, 1ull << 20, 55987200ull, (1ull << 31) - 1, 1ull << 31};
  for (uint64_t n : rows)
    for (uint32_t F = 1; F <= kGrowMaxFeatures; ++F)
      for (int cus : {1, 8, 256}) {
        const GrowPlan p = plan_grow_weighted(n, F, (uint64_t)F * kGrowMaxCuts, kGrowMaxDepth, cus);
        const GrowPlan u = plan_grow(n, F, (uint64_t)F * kGrowMaxCuts, kGrowMaxDepth, cus);
        EXPECT(p.levels.size() == (size_t)kGrowMaxDepth && p.row_blocks == u.row_blocks && p.hist_bytes == u.hist_bytes);
        for (size_t d = 0; d < p.levels.size(); ++d) {
          const GrowLevelPlan& l = p.levels[d];
          EXPECT(l.slots == (1u << d) && l.node_group >= 1 && l.feat_group >= 1);
          EXPECT(l.node_group * l.feat_group <= kGrowWeightedMaxPairs);
          EXPECT(l.lds_bytes == l.node_group * l.feat_group * kGrowWeightedPairBytes && l.lds_bytes <= kGrowLdsBytes);
          EXPECT(l.node_groups * l.node_group >= l.slots && (l.node_groups - 1) * l.node_group < l.slots);
          EXPECT(l.feat_groups * l.feat_group >= F && (l.feat_groups - 1) * l.feat_group < F);
          EXPECT(l.hist_blocks >= 1 && (uint64_t)(l.hist_blocks - 1) * kGrowHistBlock < n);
          const GrowLevelPlan& v = u.levels[d];
          EXPECT(v.node_group * v.feat_group <= kGrowMaxPairs && v.lds_bytes == v.node_group * v.feat_group * kGrowPairBytes);
        }
      }
}

static void check_sums() {
  const uint64_t top = (1ull << 63) - 1, mid = ~0ull - 0xFFFFFFFFull;   // p2, p0 < 2^63; p1 <= 2^64 - 2^32
  GrowWideSum z, a, b;
  EXPECT(grow_wide_rmse(z, 1) == 0.0);
  a.p2 = (1ull << 63) - (1ull << 33);
  a.p1 = mid;
  a.p0 = top;
  EXPECT(std::isfinite(grow_wide_rmse(a, top)) && grow_wide_rmse(a, 1) > grow_wide_rmse(a, top));
  b = a;
  b.p0 -= 1;
  EXPECT(grow_sum_less(b, a) && !grow_sum_less(a, b) && !grow_sum_less(a, a));
  // the same integer written with the carries undone
  GrowWideSum c, d;
  c.p2 = 1;
  d.p1 = 1ull << 32;
  EXPECT(!grow_sum_less(c, d) && !grow_sum_less(d, c) && grow_wide_rmse(c, 16777216) == grow_wide_rmse(d, 16777216));
  EXPECT(grow_wide_rmse(c, 16777216) == 0.0625);
  // the stop rule over wide sums
  std::vector<GrowWideSum> S(5, a);
  S[2] = b;
  uint32_t run = 0, best = 0;
  grow_eval_stop(S.data(), 4, 2, &run, &best);
  EXPECT(run == 4 && best == 2);
  grow_eval_stop(S.data(), 4, 1, &run, &best);
  EXPECT(run == 1 && best == 0);
}

static void check_splits(int histograms, uint64_t seed) {
  std::mt19937_64 rng(seed);
  for (int it = 0; it < histograms; ++it) {
    const uint32_t F = 1 + (uint32_t)(rng() % 5);
    std::vector<int64_t> G((size_t)F * kGrowBins, 0);
    std::vector<uint64_t> H((size_t)F * kGrowBins, 0);
    std::vector<uint64_t> cut_ptr(F + 1, 0);
    // every third case: sums as large as they get - 2^31 rows of |q| < 2^32 and hq < 2^32 in all
    const bool large = it % 3 == 0;
    const uint32_t rows = 2 + (uint32_t)(rng() % 300);
    std::vector<int64_t> q(rows);
    std::vector<uint64_t> hq(rows);
    int64_t Gp = 0;
    uint64_t Hp = 0;
    for (uint32_t r = 0; r < rows; ++r) {
      const uint64_t scale = large ? (1ull << 31) / rows : 1;
      q[r] = (int64_t)(rng() % (1ull << 33)) - (int64_t)(1ull << 32);
      hq[r] = rng() % 7 == 0 ? 0 : rng() % (1ull << 32);
      q[r] = (int64_t)(q[r] * (__int128)scale);
      hq[r] *= scale;
      Gp += q[r];
      Hp += hq[r];
    }
    EXPECT(Hp < (1ull << 63));
    for (uint32_t f = 0; f < F; ++f) {
      const uint32_t ncut = it % 5 == 0 ? kGrowMaxCuts : (uint32_t)(rng() % (kGrowMaxCuts + 1));
      cut_ptr[f + 1] = cut_ptr[f] + ncut;
      for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t b = rng() % 5 == 0 ? kGrowMissingBin : (uint32_t)(rng() % (ncut + 1));
        G[(size_t)f * kGrowBins + b] += q[r];
        H[(size_t)f * kGrowBins + b] += hq[r];
      }
    }
    const float lambda = it % 2 ? 0.0f : 1.0f;
    const float mcw = (float)((rng() % 4) * 0.25 * ((double)Hp / 16777216.0));
    const GrowCand c = grow_node_split(G.data(), H.data(), F, cut_ptr.data(), Gp, Hp, lambda, GrowFixedHess{(double)mcw});
    EXPECT(!std::isnan(c.loss_chg));
    if (c.valid) {
      const uint32_t f = c.key >> 9, j = (c.key >> 1) & 255u;
      EXPECT(f < F && j < cut_ptr[f + 1] - cut_ptr[f]);
      EXPECT(c.HL > 0 && c.HL < Hp && grow_hess(c.HL) >= (double)mcw && grow_hess(Hp - c.HL) >= (double)mcw);
      EXPECT(grow_weight_splits(Hp, (double)mcw));
      float leaf, w;
      grow_solve_leaf_weighted(c.GL, c.HL, 0.3f, lambda, &leaf, &w);
      EXPECT(std::isfinite(leaf) && std::isfinite(w));
      grow_solve_leaf_weighted(Gp - c.GL, Hp - c.HL, 0.3f, lambda, &leaf, &w);
      EXPECT(std::isfinite(leaf) && std::isfinite(w));
    }
  }
  // an empty child with lambda == 0: invalid, and no NaN
  std::vector<int64_t> G(kGrowBins, 0);
  std::vector<uint64_t> H(kGrowBins, 0);
  const uint64_t cut_ptr[2] = {0, 1};
  G[1] = 3 << 24;
  H[1] = 2 << 24;
  const GrowCand c = grow_node_split(G.data(), H.data(), 1, cut_ptr, G[1], H[1], 0.0f, GrowFixedHess{0.0});
  EXPECT(!c.valid && c.loss_chg == 0.0);
}

int main(int argc, char** argv) {
  const int histograms = argc > 1 ? atoi(argv[1]) : 300;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  check_plans();
  check_sums();
  check_splits(histograms, seed);
  printf("grow_weighted_host_check: %d histograms, %ld failures\n", histograms, failures);
  return failures == 0 ? 0 : 1;
}
