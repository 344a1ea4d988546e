// The host side of "ohx_reg_alpha", "ohx_max_delta_step" and "ohx_eval_metric" (csrc/grow.hpp GrowRegHess, grow_metric_row,
// grow_node_split over the policy; grow.cpp grow_wide_mean) in a program of its own, for a build with
// -fsanitize=address,undefined (CPU only; tests/test_grow_reg_cpu.py builds and runs it): the policy over crafted sums -
// G = 0, |Gd| = alpha exactly, |w| = max_delta_step exactly, alpha far above every |Gd|, H = 1 - and a node's split over
// histograms of exactly F x 256 entries; a row's term of each metric over the edges of its domain.
// Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_reg_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

static long sums = 0, rows = 0;

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

static void check_policy() {
  const int64_t one = 1ll << 24;   // Gd = 1.0
  const int64_t Gs[] = {0, 1, -1, one / 2, -one / 2, one, -one, 3 * one, -3 * one, (1ll << 40) - 1, -(1ll << 40) + 1};
  const uint64_t Hs[] = {1, (uint64_t)one / 2, (uint64_t)one, 7 * (uint64_t)one, 1ull << 40};
  const float alphas[] = {0.0f, 0.5f, 1.0f, 3.0f, 1e9f};
  const float steps[] = {0.0f, 0.25f, 0.5f, 1.0f, 100.0f};
  const float lambdas[] = {0.0f, 1.0f, 2.5f};
  for (int64_t G : Gs)
    for (uint64_t H : Hs)
      for (float lambda : lambdas)
        for (float alpha : alphas)
          for (float m : steps) {
            ++sums;
            const GrowRegHess reg{0.0, alpha, m};
            const GrowFixedHess fixed{0.0};
            const double gain = reg.gain(G, H, (double)lambda);
            float leaf = 7.0f, w = 7.0f, leaf0 = 7.0f, w0 = 7.0f;
            reg.solve_leaf(G, H, 0.125f, lambda, &leaf, &w);
            fixed.solve_leaf(G, H, 0.125f, lambda, &leaf0, &w0);
            const double Gd = (double)G / 16777216.0;
            if (alpha == 0.0f && m == 0.0f) {   // today's bits, a base_weight of -0.0f at G == 0 included
              EXPECT(same_bits(gain, fixed.gain(G, H, (double)lambda)) && same_bits(gain, grow_gain(G, grow_hess(H), (double)lambda)));
              EXPECT(same_bits(w, w0) && same_bits(leaf, leaf0));
            }
            if (G == 0) EXPECT(same_bits(w, -0.0f) && gain == 0.0);
            if (std::fabs(Gd) <= (double)alpha) EXPECT(same_bits(w, -0.0f) && gain == 0.0);   // |Gd| == alpha exactly too
            if (m > 0.0f) EXPECT(std::fabs(w) <= m);
            EXPECT(std::isfinite(gain) && gain >= 0.0);   // D > 0: H >= 1
            EXPECT(same_bits(leaf, w * 0.125f) && reg.sum_hess(H) == fixed.sum_hess(H));
            EXPECT(reg.admits(H, 1) == fixed.admits(H, 1) && reg.evaluates(H) == fixed.evaluates(H));
            // a weight of exactly m is not clipped: the unclipped form and the clipped one agree there
            if (m > 0.0f && alpha == 0.0f && std::fabs(-Gd / (grow_hess(H) + (double)lambda)) == (double)m)
              EXPECT(std::fabs(w) == m);
          }
  // |w| == m exactly: Gd = -1, D = 2 (H = 1.0, lambda = 1) gives w = 0.5 = m; one unit more of G is clipped to it
  {
    float leaf, w;
    const GrowRegHess reg{0.0, 0.0f, 0.5f};
    reg.solve_leaf(-one, (uint64_t)one, 1.0f, 1.0f, &leaf, &w);
    EXPECT(w == 0.5f);
    reg.solve_leaf(-one - 1, (uint64_t)one, 1.0f, 1.0f, &leaf, &w);
    EXPECT(w == 0.5f);
    reg.solve_leaf(-one + 1, (uint64_t)one, 1.0f, 1.0f, &leaf, &w);
    EXPECT(w < 0.5f && w > 0.49f);
    // where nothing is clipped the second gain form is the first up to rounding
    const double a = reg.gain(-one / 2, (uint64_t)one, 1.0), b = GrowRegHess{0.0, 0.0f, 0.0f}.gain(-one / 2, (uint64_t)one, 1.0);
    EXPECT(std::fabs(a - b) <= 1e-15);
  }
  EXPECT(grow_reg_sound(0.0f) && grow_reg_sound(1e30f) && !grow_reg_sound(-1.0f) && !grow_reg_sound(std::numeric_limits<float>::infinity()) &&
         !grow_reg_sound(std::numeric_limits<float>::quiet_NaN()));
}

// a node's split over histograms of exactly F x 256 entries: with alpha above every |Gd| no candidate gains anything
static void check_node_split() {
  const uint32_t F = 3;
  std::vector<int64_t> G((size_t)F * kGrowBins, 0);
  std::vector<uint64_t> H((size_t)F * kGrowBins, 0);
  const uint64_t cut_ptr[] = {0, 254, 254 + 7, 254 + 7 + 1};
  int64_t Gp = 0;
  uint64_t Hp = 0;
  for (uint32_t b = 0; b < kGrowBins; ++b) {
    const int64_t g = ((int64_t)b - 100) * (1 << 20);
    G[b] = g;
    H[b] = 1 << 24;
    Gp += g;
    Hp += 1 << 24;
  }
  for (uint32_t f = 1; f < F; ++f) {   // the other features see the same rows in other bins
    G[(size_t)f * kGrowBins + kGrowMissingBin] = Gp;
    H[(size_t)f * kGrowBins + kGrowMissingBin] = Hp;
  }
  const GrowCand plain = grow_node_split(G.data(), H.data(), F, cut_ptr, Gp, Hp, 1.0f, GrowFixedHess{0.0});
  const GrowCand same = grow_node_split(G.data(), H.data(), F, cut_ptr, Gp, Hp, 1.0f, GrowRegHess{0.0, 0.0f, 0.0f});
  EXPECT(plain.valid && same.valid && plain.key == same.key && same_bits(plain.loss_chg, same.loss_chg) && plain.GL == same.GL &&
         plain.HL == same.HL);
  const GrowCand far = grow_node_split(G.data(), H.data(), F, cut_ptr, Gp, Hp, 1.0f, GrowRegHess{0.0, 1e9f, 0.0f});
  EXPECT(far.valid && far.loss_chg == 0.0 && far.key == grow_key(0, 0, 0));   // every gain is 0: the smallest key stays
  const GrowCand clipped = grow_node_split(G.data(), H.data(), F, cut_ptr, Gp, Hp, 1.0f, GrowRegHess{0.0, 0.5f, 0.25f});
  EXPECT(clipped.valid && std::isfinite(clipped.loss_chg));
  EXPECT(!grow_node_split(G.data(), H.data(), F, cut_ptr, Gp, Hp, 1.0f, GrowRegHess{1e9, 0.5f, 0.25f}).valid);   // min_child_weight
}

static void check_metric() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float below = std::nextafterf(256.0f, 0.0f);
  const float zs[] = {0.0f, -0.0f, 0x1p-149f, -0x1p-149f, 0x1p-130f, 0x1p-126f, 0x1p-70f, -0x1p-70f, 0x1p-25f, 0x1p-24f, 1e-3f, 0.5f,
                      -1.0f, 3.7f, 100.0f, -200.0f, below, -below, 256.0f, -256.0f, 1e30f, inf, -inf, nan};
  const float slopes[] = {kGrowMinSlope, 0.5f, 1.0f, 3.7f, kGrowMaxSlope};
  for (uint32_t metric : {kGrowMetricRmse, kGrowMetricMae, kGrowMetricPseudoHuber})
    for (float slope : slopes)
      for (float z : zs) {
        ++rows;
        uint64_t sq = 77;
        const bool sound = grow_metric_row_of(metric, slope, z, 0.0f, &sq);   // pred - label == z exactly
        EXPECT(sound == (std::fabs(z) < 256.0f));
        if (!sound) {
          EXPECT(sq == 0);
          continue;
        }
        const uint64_t e = (uint64_t)std::llabs((long long)std::rint((double)z * 16777216.0));
        if (metric == kGrowMetricRmse) EXPECT(sq == e * e);
        if (metric == kGrowMetricMae) EXPECT(sq == e && sq < (1ull << 32));
        if (metric == kGrowMetricPseudoHuber) {
          EXPECT(sq < (1ull << 40));
          // mf <= delta |z| and mf <= z^2 / 2, up to the rounding of four float32 operations
          EXPECT((double)sq <= ((double)slope * std::fabs((double)z)) * 16777216.0 * 1.000001 + 1.0);
          EXPECT((double)sq <= ((double)z * (double)z / 2.0) * 16777216.0 * 1.000001 + 1.0);
        }
        if (std::fabs(z) < 0x1p-70f) EXPECT(sq == 0);   // zero, denormals: nothing, flushed or not
      }
  // the reported value of mae and pseudohuber: S * 2^-48 over W * 2^-24, no square root
  GrowWideSum s;
  s.p1 = 3;   // S = 3 * 2^32
  EXPECT(grow_wide_mean(s, 1ull << 24) == 3.0 / 65536.0);
  s.p2 = 1;
  s.p1 = 0;   // S = 2^64
  EXPECT(grow_wide_mean(s, 1ull << 25) == 32768.0);
}

int main() {
  check_policy();
  check_node_split();
  check_metric();
  printf("grow_reg_host_check: %ld sums, %ld rows, %ld failures\n", sums, rows, failures);
  return failures == 0 ? 0 : 1;
}
