// The host side of quantile boosting (csrc/grow_quantile.hpp: the rule, the pick of a digit, the leaf value; csrc/grow.hpp:
// the quantile pair and the pinball term) in a program of its own, for a build with -fsanitize=address,undefined (CPU only;
// tests/test_grow_quantile_cpu.py builds and runs it): the four-pass select over leaves of crafted and random keys and
// weights, in bins of exactly 256 entries, against a sort; the coverage property of every pick; the pair and the metric
// term over the edges of their domain.  Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_quantile_host_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <utility>
#include <vector>

#include "grow.hpp"
#include "grow_quantile.hpp"

using namespace ohx;

static long failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      ++failures;                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);            \
    }                                                            \
  } while (0)

static long selects = 0, rows_seen = 0;

static uint64_t next_random(uint64_t* s) { return *s = grow_mix(*s + kGrowGamma64); }

// one leaf: the radix select over (residual, hq) against the sorted rule
static void check_leaf(const std::vector<float>& r, const std::vector<uint32_t>& hq, float alpha) {
  ++selects;
  rows_seen += (long)r.size();
  const uint32_t alpha_q = grow_alpha_q(alpha);
  EXPECT(alpha_q >= (1u << 14) && alpha_q <= (1u << 24) - (1u << 14));
  GrowQuantileLeaf leaf;
  bool live = true;
  for (uint32_t pass = 0; pass < kGrowQuantilePasses && live; ++pass) {
    std::vector<uint64_t> bins(kGrowQuantileDigits, 0);   // exactly 256 entries
    for (size_t i = 0; i < r.size(); ++i) {
      if (hq[i] == 0) continue;
      const uint32_t k = grow_quantile_key(0.0f, r[i]);   // label - 0 is r itself
      if (grow_quantile_matches(k, leaf.prefix, pass)) bins[grow_quantile_digit(k, pass)] += hq[i];
    }
    live = grow_quantile_pick(bins.data(), pass, alpha_q, &leaf);
  }
  std::vector<std::pair<uint32_t, uint64_t>> rows;
  unsigned __int128 W = 0;
  for (size_t i = 0; i < r.size(); ++i)
    if (hq[i] != 0) {
      rows.push_back({cuts_key(cuts_float_bits(r[i])), hq[i]});
      W += hq[i];
    }
  EXPECT(live == (W != 0));
  if (!live || W == 0) return;
  EXPECT((unsigned __int128)leaf.W == W);
  std::sort(rows.begin(), rows.end());
  unsigned __int128 C = 0, below = 0;
  uint32_t want = 0;
  bool found = false;
  for (size_t i = 0; i < rows.size() && !found; ++i) {
    if (i == 0 || rows[i].first != rows[i - 1].first) below = C;
    C += rows[i].second;
    if ((i + 1 == rows.size() || rows[i + 1].first != rows[i].first) && (unsigned __int128)alpha_q * W <= (C << 24)) {
      want = rows[i].first;
      found = true;
    }
  }
  EXPECT(found && leaf.prefix == want);
  EXPECT((unsigned __int128)leaf.below == below);
  EXPECT((below << 24) < (unsigned __int128)alpha_q * W && (unsigned __int128)alpha_q * W <= (C << 24));
  const float v = grow_quantile_value(leaf.prefix, 1.0f);
  EXPECT(cuts_key(cuts_float_bits(v)) == want);
}

int main() {
  const float alphas[] = {kGrowMinAlpha, 0.05f, 0.5f, 0.95f, kGrowMaxAlpha};
  const float below = std::nextafterf(256.0f, 0.0f);
  const uint32_t heavy = (uint32_t)std::rint((double)below * 16777216.0);
  for (float alpha : alphas) {
    check_leaf({1.5f}, {1u << 24}, alpha);
    check_leaf({1.5f}, {0u}, alpha);
    check_leaf({}, {}, alpha);
    check_leaf({2.0f, 2.0f, 2.0f, 2.0f}, {1, 2, 3, heavy}, alpha);
    check_leaf({0.0f, -0.0f, 0.0f, -0.0f}, {5, 5, 5, 5}, alpha);
    check_leaf({-3.0f, 3.0f, -0x1p-149f, 0x1p-149f, -below, below}, {7, 7, 7, 7, 7, 7}, alpha);
    std::vector<float> low, high;
    std::vector<uint32_t> w;
    for (uint32_t i = 0; i < 256; ++i) {
      low.push_back(__builtin_bit_cast(float, 0x3F800000u + i));              // the lowest 8 key bits
      high.push_back(__builtin_bit_cast(float, ((i & 127u) << 24) | ((i >> 7) << 31) | 0x00400000u));   // the highest
      w.push_back(i % 3 == 0 ? 0u : i % 3 == 1 ? 1u : heavy);
    }
    for (float& v : high)
      if (!(std::fabs(v) < 256.0f)) v = 1.0f;
    check_leaf(low, w, alpha);
    check_leaf(high, w, alpha);
    uint64_t s = 32;
    std::vector<float> r;
    std::vector<uint32_t> h;
    for (int i = 0; i < 20000; ++i) {
      const uint64_t a = next_random(&s);
      r.push_back(((float)(a >> 40) * 0x1p-24f - 0.5f) * ((a & 1) ? 400.0f : 0x1p-100f));
      h.push_back((a & 6) == 0 ? 0u : (uint32_t)(next_random(&s) >> 32));
    }
    check_leaf(r, h, alpha);
  }
  // the pair and the pinball term
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (float alpha : alphas)
    for (float z : {0.0f, -0.0f, 0x1p-149f, -0x1p-149f, 1.0f, -1.0f, below, -below, 256.0f, nan})
      for (float w : {0.0f, 0x1p-24f, 1.0f, below, 256.0f, -1.0f}) {
        int64_t q = 77;
        uint32_t hq = 77;
        const uint32_t flags = grow_pair_of(kGrowObjQuantile, alpha, z, 0.0f, w, &q, &hq);
        const bool z_sound = std::fabs(z) < 256.0f, w_sound = w >= 0.0f && w < 256.0f;
        if (!z_sound) EXPECT(flags == kGrowFlagLabel && q == 0 && hq == 0);
        else if (!w_sound) EXPECT(flags == kGrowFlagWeight && q == 0 && hq == 0);
        else {
          EXPECT(flags == 0 && hq == (uint32_t)std::rint((double)w * 16777216.0));
          EXPECT(z >= 0.0f ? q >= 0 : q <= 0);
          if (w == 1.0f) EXPECT(q == (z >= 0.0f ? (int64_t)(1u << 24) - (int64_t)grow_alpha_q(alpha) : -(int64_t)grow_alpha_q(alpha)));
        }
        uint64_t sq = 77;
        const bool sound = grow_metric_row_of(kGrowMetricQuantile, alpha, z, 0.0f, &sq);
        EXPECT(sound == z_sound && (sound || sq == 0) && sq < (1ull << 56));
      }
  EXPECT(!grow_alpha_sound(0.0f) && !grow_alpha_sound(1.0f) && !grow_alpha_sound(nan) && grow_alpha_sound(0.5f) &&
         grow_alpha_sound(kGrowMinAlpha) && grow_alpha_sound(kGrowMaxAlpha) && !grow_alpha_sound(std::nextafterf(kGrowMinAlpha, 0.0f)));
  EXPECT(grow_quantile_reached(1u << 24, (1ull << 63) - 1, (1ull << 63) - 1) && !grow_quantile_reached(1u << 24, (1ull << 63) - 1, (1ull << 63) - 2));
  printf("grow_quantile_host_check: %ld selects, %ld rows, %ld failures\n", selects, rows_seen, failures);
  return failures == 0 ? 0 : 1;
}
