// The host functions of column sampling by level and by node (csrc/grow.hpp, grow.cpp) in a program of their own, for a
// build with -fsanitize=address,undefined (CPU only; tests/test_grow_colsample_cpu.py builds and runs it): the level and
// node keys with wrapping seeds and tree indices, the order of two draws with equal keys, the lists of a level and of a
// node into buffers of exactly n_lvl and n_node bytes, their nesting, and the rank a split kernel computes against the
// node's list.  Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_colsample_host_check [draws] [seed]
#include <algorithm>
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
  const uint64_t top = ~0ull;
  const uint64_t col = grow_col_key(top, 1ull << 63);
  EXPECT(grow_level_key(col, 0) == grow_mix(col + kGrowGamma64));
  EXPECT(grow_level_key(col, 17) == grow_mix(col + kGrowGamma64 * 18));
  EXPECT(grow_node_key(col, 0) == grow_mix(col + kGrowGamma64 * 32));
  EXPECT(grow_node_key(col, (1u << 19) - 1) == grow_mix(col + kGrowGamma64 * (32ull + (1u << 19) - 1)));
  EXPECT(grow_node_key(col, ~0u) == grow_mix(col + kGrowGamma64 * (32ull + ~0u)));   // (no 32-bit wrap)
  for (uint32_t d = 0; d < 18; ++d)
    for (uint32_t p = 0; p < 64; ++p) EXPECT(grow_level_key(col, d) != grow_node_key(col, p));
  // equal keys order by the feature; unequal keys by the key alone
  EXPECT(grow_draw_below(5, 3, 5, 7) && !grow_draw_below(5, 7, 5, 3) && !grow_draw_below(5, 3, 5, 3));
  EXPECT(grow_draw_below(4, 9, 5, 3) && !grow_draw_below(6, 1, 5, 3));
}

static void check_refusals() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const uint8_t list[3] = {1, 5, 9};
  uint8_t guard[4] = {77, 77, 77, 77};
  for (float bad : {nan, inf, -inf, 0.0f, -1.0f, 1.5f}) {
    EXPECT(grow_pick_level_features(1, 2, 3, list, 3, bad, guard) == 0 && guard[0] == 77);
    EXPECT(grow_pick_node_features(1, 2, 3, list, 3, bad, guard) == 0 && guard[0] == 77);
  }
  EXPECT(grow_pick_level_features(1, 2, 3, list, 0, 0.5f, guard) == 0 && guard[0] == 77);
  EXPECT(grow_pick_level_features(1, 2, 3, list, kGrowMaxFeatures + 1, 0.5f, guard) == 0 && guard[0] == 77);
  // 0.34f of 3 is 1; 0.99f of 1 is 1 and draws nothing
  EXPECT(grow_pick_level_features(1, 2, 3, list, 3, 0.34f, guard) == 1 && guard[1] == 77);
  EXPECT(grow_pick_level_features(1, 2, 3, list, 1, 0.99f, guard) == 1 && guard[0] == 1 && guard[1] == 77);
  EXPECT(grow_pick_node_features(1, 2, 3, list, 3, 1.0f, guard) == 3 && guard[0] == 1 && guard[1] == 5 && guard[2] == 9 && guard[3] == 77);
}

static long lists = 0, ranks = 0;

static void check_draws(int draws, uint64_t seed0) {
  std::mt19937_64 rng(seed0);
  for (int it = 0; it < draws; ++it) {
    const uint64_t seed = it % 4 == 0 ? ~0ull - (uint64_t)it : rng(), tree = it % 3 == 0 ? rng() : (uint64_t)(it % 7);
    const uint32_t n_sel = it % 11 == 0 ? kGrowMaxFeatures : 1 + (uint32_t)(rng() % kGrowMaxFeatures);
    const float bylevel = it % 5 == 0 ? 1.0f : (float)((rng() % 1000 + 1) / 1000.0);
    const float bynode = it % 7 == 0 ? 1.0f : (float)((rng() % 1000 + 1) / 1000.0);
    const uint32_t level = (uint32_t)(rng() % 18), node = (uint32_t)(rng() % (1u << 19));
    // a tree's list: n_sel of 128, ascending, in a buffer of its own size
    std::vector<uint8_t> all(kGrowMaxFeatures);
    for (uint32_t f = 0; f < kGrowMaxFeatures; ++f) all[f] = (uint8_t)f;
    std::shuffle(all.begin(), all.end(), rng);
    std::vector<uint8_t> tree_list(all.begin(), all.begin() + n_sel);
    std::sort(tree_list.begin(), tree_list.end());
    const uint32_t n_lvl = grow_num_selected(n_sel, bylevel);
    std::vector<uint8_t> lvl(n_lvl);
    EXPECT(grow_pick_level_features(seed, tree, level, tree_list.data(), n_sel, bylevel, lvl.data()) == n_lvl);
    ++lists;
    for (uint32_t k = 0; k < n_lvl; ++k) {
      EXPECT(k == 0 || lvl[k - 1] < lvl[k]);
      EXPECT(std::binary_search(tree_list.begin(), tree_list.end(), lvl[k]));
    }
    if (n_lvl == n_sel) EXPECT(lvl == tree_list);
    if (n_lvl < n_sel) {   // no feature left out has a smaller (key, f) than one taken
      const uint64_t key = grow_level_key(grow_col_key(seed, tree), level);
      for (uint8_t out : tree_list) {
        if (std::binary_search(lvl.begin(), lvl.end(), out)) continue;
        for (uint8_t in : lvl) EXPECT(grow_draw_below(grow_mix(key + in), in, grow_mix(key + out), out));
      }
    }
    const uint32_t n_node = grow_num_selected(n_lvl, bynode);
    std::vector<uint8_t> mine(n_node);
    EXPECT(grow_pick_node_features(seed, tree, node, lvl.data(), n_lvl, bynode, mine.data()) == n_node);
    ++lists;
    for (uint32_t k = 0; k < n_node; ++k) EXPECT(k == 0 || mine[k - 1] < mine[k]);
    // the rank names the same set
    for (uint8_t f : lvl) {
      EXPECT(grow_node_has_feature(seed, tree, node, lvl.data(), n_lvl, n_node, f) == std::binary_search(mine.begin(), mine.end(), f));
      ++ranks;
    }
  }
}

int main(int argc, char** argv) {
  const int draws = argc > 1 ? atoi(argv[1]) : 3000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 29;
  check_keys();
  check_refusals();
  check_draws(draws, seed);
  printf("%ld lists, %ld ranks, %ld failures\n", lists, ranks, failures);
  return failures == 0 ? 0 : 1;
}
