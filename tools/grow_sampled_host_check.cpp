// The host functions of boosting with row and column subsampling (csrc/grow.hpp, grow.cpp) in a program of their own,
// for a build with -fsanitize=address,undefined (CPU only; tests/test_grow_sampled_cpu.py builds and runs it): the mix
// function and the tree keys with wrapping seeds and tree indices, the threshold and n_sel at the edges of their
// arguments, the bag, the selected features into a buffer of exactly n_sel bytes, and the plan over n_sel features.
// Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_sampled_host_check <draws> <seed>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

static void check_keys() {
  // splitmix64's finalizer: known values of the sequence seeded with 0 (state += gamma64, then mix)
  EXPECT(grow_mix(0) == 0);
  EXPECT(grow_mix(kGrowGamma64) == 0xE220A8397B1DCDAFull);
  EXPECT(grow_mix(2 * kGrowGamma64) == 0x6E789E6AA1B965F4ull);
  EXPECT(grow_row_key(0, 0) == grow_mix(kGrowGamma64) && grow_col_key(0, 0) == grow_mix(2 * kGrowGamma64));
  // seeds and tree indices that wrap
  const uint64_t top = ~0ull;
  EXPECT(grow_row_key(top, top) == grow_mix(top + kGrowGamma64 * (2 * top + 1)));
  EXPECT(grow_col_key(top, (1ull << 63)) == grow_mix(top + kGrowGamma64 * 2));
  EXPECT(grow_row_key(5, 1ull << 32) != grow_row_key(5, 0));
}

static void check_thresholds() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  for (float bad : {nan, inf, -inf, 0.0f, -0.0f, -1.0f, std::nextafter(1.0f, 2.0f), 2.0f, 3e38f}) {
    EXPECT(grow_sample_threshold(bad) == 0);
    EXPECT(grow_num_selected(27, bad) == 0);
  }
  EXPECT(grow_sample_threshold(1.0f) == kGrowSampleOne && grow_sample_threshold(0.5f) == (1u << 23));
  EXPECT(grow_sample_threshold(std::nextafter(1.0f, 0.0f)) == kGrowSampleOne - 1);
  EXPECT(grow_sample_threshold(0x1p-24f) == 1 && grow_sample_threshold(0x1p-25f) == 0);   // the tie rounds to even
  EXPECT(grow_sample_threshold(0x1.8p-25f) == 1 && grow_sample_threshold(std::numeric_limits<float>::denorm_min()) == 0);
  EXPECT(grow_num_selected(3, 0.34f) == 1 && grow_num_selected(3, 0.33f) == 1 && grow_num_selected(3, 0.67f) == 2);
  EXPECT(grow_num_selected(128, 0x1p-20f) == 1 && grow_num_selected(128, 1.0f) == 128 && grow_num_selected(1, 0.01f) == 1);
  EXPECT(grow_num_selected(0, 0.5f) == 0 && grow_num_selected(27, 0.5f) == 13);
}

static void check_draws(int draws, uint64_t seed0) {
  std::mt19937_64 rng(seed0);
  for (int it = 0; it < draws; ++it) {
    const uint64_t seed = it % 4 == 0 ? ~0ull - (uint64_t)it : rng(), tree = it % 3 == 0 ? rng() : (uint64_t)(it % 7);
    const uint32_t F = 1 + (uint32_t)(rng() % kGrowMaxFeatures);
    const float colsample = it % 5 == 0 ? 1.0f : (float)((rng() % 1000 + 1) / 1000.0);
    const uint32_t n_sel = grow_num_selected(F, colsample);
    EXPECT(n_sel >= 1 && n_sel <= F);
    std::vector<uint8_t> out(n_sel);   // exactly n_sel bytes: a write past them is caught
    EXPECT(grow_pick_features(seed, tree, F, colsample, out.data()) == n_sel);
    for (uint32_t k = 0; k < n_sel; ++k) EXPECT(out[k] < F && (k == 0 || out[k - 1] < out[k]));
    if (n_sel < F) {
      // no feature left out has a smaller (key, f) than one taken
      const uint64_t key = grow_col_key(seed, tree);
      std::vector<bool> in(F, false);
      for (uint8_t f : out) in[f] = true;
      uint64_t worst_in = 0, best_out = ~0ull;
      for (uint32_t f = 0; f < F; ++f) {
        const uint64_t c = grow_mix(key + f);
        if (in[f]) worst_in = c > worst_in ? c : worst_in;
        else best_out = c < best_out ? c : best_out;
      }
      EXPECT(worst_in <= best_out);
    }
    // the bag: the fraction over 2^16 rows lies within 6 sigma of k_s / 2^24
    const float subsample = (float)((rng() % 1000 + 1) / 1000.0);
    const uint32_t k_s = grow_sample_threshold(subsample);
    EXPECT(k_s >= 1 && k_s <= kGrowSampleOne);
    const uint64_t key = grow_row_key(seed, tree), first = it % 2 ? 0 : (1ull << 31) - 65536;
    uint32_t in_bag = 0;
    for (uint64_t r = 0; r < 65536; ++r) in_bag += grow_in_bag(key, first + r, k_s) ? 1u : 0u;
    const double p = (double)k_s / 16777216.0, sigma = std::sqrt(p * (1.0 - p) / 65536.0);
    EXPECT(std::fabs(in_bag / 65536.0 - p) <= 6.0 * sigma + 1e-12);
  }
  // refused arguments write nothing
  uint8_t guard[1] = {77};
  EXPECT(grow_pick_features(1, 2, 27, 0.0f, guard) == 0 && guard[0] == 77);
  EXPECT(grow_pick_features(1, 2, kGrowMaxFeatures + 1, 0.5f, guard) == 0 && guard[0] == 77);
}

static void check_plans() {
  const uint64_t rows[] = {1, 63, 4097, 55987200ull, 1ull << 31};
  for (uint64_t n : rows)
    for (uint32_t n_sel = 1; n_sel <= kGrowMaxFeatures; ++n_sel) {
      const GrowPlan p = plan_grow_weighted(n, n_sel, 0, kGrowMaxDepth, 256);
      EXPECT(p.levels.size() == (size_t)kGrowMaxDepth);
      EXPECT(p.hist_bytes == (uint64_t)(1u << (kGrowMaxDepth - 1)) * n_sel * kGrowBins * 16);
      for (const GrowLevelPlan& l : p.levels) {
        EXPECT(l.node_group * l.feat_group <= kGrowWeightedMaxPairs && l.lds_bytes <= kGrowLdsBytes);
        EXPECT(l.feat_groups * l.feat_group >= n_sel && (l.feat_groups - 1) * l.feat_group < n_sel);
      }
    }
}

int main(int argc, char** argv) {
  const int draws = argc > 1 ? atoi(argv[1]) : 200;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  check_keys();
  check_thresholds();
  check_draws(draws, seed);
  check_plans();
  printf("grow_sampled_host_check: %d draws, %ld failures\n", draws, failures);
  return failures == 0 ? 0 : 1;
}
