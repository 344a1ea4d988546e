// The two host decisions behind the clustering pass and the level search (csrc/kernels.hpp cluster_order and
// pick_level_period) in a program of their own, for a build with -fsanitize=address,undefined (CPU only;
// tests/test_cluster_cpu.py builds and runs it): the nine words and the verdict words come from heap buffers of exactly
// their size, so a read past either end is reported; row counts up to 2^40; every verdict pattern of small searches
// against a search written the other way round.  Exits 0 and prints "0 failures" when every invariant holds.
// usage: cluster_host_check [draws] [seed]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "kernels.hpp"

using namespace ohx;

static long failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      ++failures;                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);            \
    }                                                            \
  } while (0)

static long orders = 0, picks = 0;

static void check_order(int draws, std::mt19937_64& rng) {
  for (int it = 0; it < draws; ++it) {
    const uint64_t nrow = it % 5 == 0 ? 0xFFFFFFF0ull : 1 + rng() % (it % 2 ? 1000 : 1u << 30);
    std::vector<uint32_t> h(9, 0u);          // exactly nine words
    uint64_t left = nrow;
    for (int v = 1; v <= 8; ++v) {
      const uint64_t take = v == 8 ? left : (it % 3 == 0 ? (v == 1 + it % 8 ? left : 0) : rng() % (left + 1));
      h[v] = (uint32_t)take;
      left -= take;
    }
    const uint64_t pairs = nrow - (nrow + 63) / 64;                 // rows that have a neighbour in their wave
    h[0] = (uint32_t)(pairs ? rng() % (pairs + 1) : 0);
    double observed = -1.0, by_chance = -1.0;
    const double order = cluster_order(h.data(), nrow, &observed, &by_chance);
    ++orders;
    EXPECT(observed >= 0.0 && observed < 1.0 + 1e-12);
    EXPECT(by_chance >= 0.125 - 1e-12 && by_chance <= 1.0 + 1e-12);
    EXPECT(std::isfinite(order) && order <= 1.0 + 1e-9);
    if (by_chance >= 0.999) EXPECT(order == 0.0);
    else EXPECT(std::fabs(order * (1.0 - by_chance) - (observed - by_chance)) <= 1e-12);
    EXPECT(cluster_order(h.data(), nrow, nullptr, nullptr) == order);       // the two outputs are optional
  }
  // the rule's constant, and its direction: rows in no order are clustered, ordered rows are left
  const uint32_t shuffled[9] = {1250, 1250, 1250, 1250, 1250, 1250, 1250, 1250, 1250};
  const uint32_t sorted[9] = {9800, 1250, 1250, 1250, 1250, 1250, 1250, 1250, 1250};
  EXPECT(kClusterOrderBelow == 0.33);
  EXPECT(cluster_order(shuffled, 10000, nullptr, nullptr) < kClusterOrderBelow);
  EXPECT(cluster_order(sorted, 10000, nullptr, nullptr) >= kClusterOrderBelow);
}

// the same rule from the other end: per column the largest k whose word is 0 and whose period fits an int
static uint64_t pick_naive(const std::vector<uint32_t>& v, uint32_t kmax, uint64_t nrow) {
  for (uint32_t c = 0; c < 4; ++c) {
    uint64_t best = 0;
    for (uint32_t k = 2; k <= kmax; ++k)
      if (v[(size_t)c * (kmax - 1) + (kmax - k)] == 0 && nrow / k <= 0x7FFFFFFFull) best = nrow / k;
    if (best) return best;
  }
  return 0;
}

static void check_pick(int draws, std::mt19937_64& rng) {
  // every pattern of {0, 1, 2} for kmax = 2 (one word a column) and kmax = 3
  for (uint32_t kmax = 2; kmax <= 3; ++kmax) {
    const size_t words = (size_t)4 * (kmax - 1);
    size_t patterns = 1;
    for (size_t i = 0; i < words; ++i) patterns *= 3;
    for (size_t p = 0; p < patterns; ++p) {
      std::vector<uint32_t> v(words);        // exactly 4 x (kmax - 1) words
      size_t q = p;
      for (size_t i = 0; i < words; ++i, q /= 3) v[i] = (uint32_t)(q % 3);
      for (uint64_t nrow : {(uint64_t)8192 * 6, (uint64_t)1 << 33, (uint64_t)3 << 31}) {
        EXPECT(pick_level_period(v.data(), kmax, nrow) == pick_naive(v, kmax, nrow));
        ++picks;
      }
    }
  }
  for (int it = 0; it < draws; ++it) {
    const uint32_t kmax = it % 7 == 0 ? 1024u : 2u + (uint32_t)(rng() % 40);
    const uint64_t nrow = it % 3 == 0 ? (uint64_t)1 << (31 + rng() % 10) : 4096ull * kmax + rng() % 100000;
    std::vector<uint32_t> v((size_t)4 * (kmax - 1));
    const uint32_t zero_one_in = 1 + (uint32_t)(rng() % 50);
    for (uint32_t& w : v) w = rng() % zero_one_in == 0 ? 0u : 1u + (uint32_t)(rng() % 2);
    const uint64_t got = pick_level_period(v.data(), kmax, nrow);
    EXPECT(got == pick_naive(v, kmax, nrow));
    EXPECT(got <= 0x7FFFFFFFull);
    ++picks;
  }
}

int main(int argc, char** argv) {
  const int draws = argc > 1 ? atoi(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 30);
  check_order(draws, rng);
  check_pick(draws, rng);
  printf("%ld orders, %ld picks, %ld failures\n", orders, picks, failures);
  return failures == 0 ? 0 : 1;
}
