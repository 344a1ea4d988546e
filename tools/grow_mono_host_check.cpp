// The host side of "ohx_monotone_constraints" (csrc/grow.hpp GrowMonoHess, grow_gain_at, the constrained grow_best_split
// and grow_mono_node_split) in a program of its own, for a build with -fsanitize=address,undefined (CPU only;
// tests/test_grow_mono_cpu.py builds and runs it): the weight under an interval over crafted sums - G = 0 and its -0.0, a
// weight clamped at either end, an interval of one point - the children's intervals, and a node's split over histograms of
// exactly F x 256 entries and exactly F constraints, where every winner must respect its feature's direction.
// Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_mono_host_check
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

static long sums = 0, nodes = 0;
static const double kInf = std::numeric_limits<double>::infinity();

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

static void check_policy() {
  const int64_t one = 1ll << 24;   // Gd = 1.0
  const int64_t Gs[] = {0, 1, -1, one / 2, -one / 2, one, -one, 3 * one, -3 * one, (1ll << 40) - 1, -(1ll << 40) + 1};
  const uint64_t Hs[] = {1, (uint64_t)one / 2, (uint64_t)one, 7 * (uint64_t)one, 1ull << 40};
  const float alphas[] = {0.0f, 0.5f, 3.0f};
  const float steps[] = {0.0f, 0.5f, 100.0f};
  const double ends[] = {-kInf, -2.0, -0.25, -0.0, 0.0, 0.25, 2.0, kInf};
  for (int64_t G : Gs)
    for (uint64_t H : Hs)
      for (float alpha : alphas)
        for (float m : steps)
          for (double lo : ends)
            for (double hi : ends) {
              if (lo > hi || lo == kInf || hi == -kInf) continue;   // (an end is infinite only where it is the root's)
              ++sums;
              const GrowRegHess reg{0.0, alpha, m};
              const GrowMonoHess h{reg, lo, hi, 0};
              const double free_w = grow_reg_weight((double)G / 16777216.0, grow_hess(H) + 1.0, (double)alpha, (double)m);
              const double w = h.weight(G, H, 1.0);
              EXPECT(w >= lo && w <= hi);
              if (free_w >= lo && free_w <= hi) EXPECT(same_bits(w, free_w));   // -0.0 stays -0.0 at lo = +0.0
              if (free_w < lo) EXPECT(same_bits(w, lo));
              if (free_w > hi) EXPECT(same_bits(w, hi));
              if (lo == hi) EXPECT(w == lo);                                    // an interval of one point
              // the whole line is the regularised policy, bit for bit, where nothing can be clipped by the gain's form
              if (lo == -kInf && hi == kInf) {
                float leaf, b, leaf0, b0;
                h.solve_leaf(G, H, 0.125f, 1.0f, &leaf, &b);
                reg.solve_leaf(G, H, 0.125f, 1.0f, &leaf0, &b0);
                EXPECT(same_bits(leaf, leaf0) && same_bits(b, b0));
                if (m > 0.0f) EXPECT(same_bits(h.gain(G, H, 1.0), reg.gain(G, H, 1.0)));
              }
              // gain_w at the node's own weight is the most any weight of the interval gives
              const double g = h.gain(G, H, 1.0);
              EXPECT(std::isfinite(g));
              for (double other : {lo, hi, 0.5 * (std::fmax(lo, -8.0) + std::fmin(hi, 8.0))})
                if (std::isfinite(other) && other >= lo && other <= hi && (m == 0.0f || std::fabs(other) <= m))
                  EXPECT(grow_gain_at((double)G / 16777216.0, grow_hess(H) + 1.0, (double)alpha, other) <= g + 1e-9 * (1.0 + std::fabs(g)));
              // the children's intervals
              for (int c : {-1, 0, 1}) {
                GrowMonoHess hc = h;
                hc.c = c;
                double iv[4];
                hc.children(G, H, -G, H, 1.0, iv);
                const double wL = hc.weight(G, H, 1.0), wR = hc.weight(-G, H, 1.0), mid = (wL + wR) * 0.5;
                if (c == 0) EXPECT(same_bits(iv[0], lo) && same_bits(iv[1], hi) && same_bits(iv[2], lo) && same_bits(iv[3], hi));
                if (c > 0) EXPECT(same_bits(iv[0], lo) && same_bits(iv[1], mid) && same_bits(iv[2], mid) && same_bits(iv[3], hi));
                if (c < 0) EXPECT(same_bits(iv[0], mid) && same_bits(iv[1], hi) && same_bits(iv[2], lo) && same_bits(iv[3], mid));
                EXPECT(hc.ordered(wL, wR) == (c == 0 || (c > 0 ? wL <= wR : wL >= wR)));
                EXPECT(hc.ordered(wL, wL));   // wL == wR is in order either way
              }
            }
}

static void check_node_split() {
  const uint32_t F = 3;
  const uint64_t cut_ptr[F + 1] = {0, 254, 261, 262};
  std::vector<int64_t> G((size_t)F * kGrowBins);
  std::vector<uint64_t> H((size_t)F * kGrowBins);
  uint64_t state = 28;
  auto draw = [&]() { return state = grow_mix(state + kGrowGamma64); };
  for (int round = 0; round < 60; ++round) {
    std::fill(G.begin(), G.end(), 0);
    std::fill(H.begin(), H.end(), 0);
    int64_t Gp = 0;
    uint64_t Hp = 0;
    for (int r = 0; r < 300; ++r) {
      const int64_t q = (int64_t)(draw() >> 38) - (1ll << 25);
      const uint64_t hq = draw() >> 39;
      for (uint32_t f = 0; f < F; ++f) {
        const uint32_t ncut = (uint32_t)(cut_ptr[f + 1] - cut_ptr[f]);
        const uint32_t b = draw() % 10 == 0 ? kGrowMissingBin : (uint32_t)(draw() % (ncut + 1));
        G[(size_t)f * kGrowBins + b] += q;
        H[(size_t)f * kGrowBins + b] += hq;
      }
      Gp += q;
      Hp += hq;
    }
    const GrowRegHess reg{round % 3 == 0 ? 2.0 : 0.0, round % 2 ? 0.5f : 0.0f, round % 4 < 2 ? 0.5f : 0.0f};
    for (int8_t c0 : {(int8_t)-1, (int8_t)0, (int8_t)1})
      for (int8_t c2 : {(int8_t)-1, (int8_t)1}) {
        ++nodes;
        const std::vector<int8_t> cons = {c0, 0, c2};   // exactly F entries
        const double lo = round % 5 == 0 ? -0.125 : -kInf, hi = round % 7 == 0 ? 0.125 : kInf;
        double iv[4] = {7, 7, 7, 7};
        const GrowCand best = grow_mono_node_split(G.data(), H.data(), F, cut_ptr, Gp, Hp, 1.0f, reg, lo, hi, cons.data(), iv);
        if (!best.valid) {
          EXPECT(iv[0] == lo && iv[1] == hi && iv[2] == lo && iv[3] == hi);
          continue;
        }
        const uint32_t f = best.key >> 9;
        EXPECT(f < F && ((best.key >> 1) & 255u) < cut_ptr[f + 1] - cut_ptr[f]);
        const GrowMonoHess h{reg, lo, hi, cons[f]};
        const double wL = h.weight(best.GL, best.HL, 1.0), wR = h.weight(Gp - best.GL, Hp - best.HL, 1.0);
        EXPECT(h.ordered(wL, wR) && h.admits(best.HL, Hp - best.HL));
        // the children's weights lie in the children's own intervals, which lie in the parent's
        EXPECT(wL >= iv[0] && wL <= iv[1] && wR >= iv[2] && wR <= iv[3]);
        EXPECT(iv[0] >= lo && iv[1] <= hi && iv[2] >= lo && iv[3] <= hi);
        const GrowMonoHess left{reg, iv[0], iv[1], 0}, right{reg, iv[2], iv[3], 0};
        EXPECT(same_bits(left.weight(best.GL, best.HL, 1.0), wL) && same_bits(right.weight(Gp - best.GL, Hp - best.HL, 1.0), wR));
        // with no constraint anywhere and the whole line, under a step, the winner is the regularised policy's
        if (c0 == 0 && lo == -kInf && hi == kInf && reg.max_delta_step > 0.0f) {
          const std::vector<int8_t> none = {0, 0, 0};
          double unused[4];
          const GrowCand a = grow_mono_node_split(G.data(), H.data(), F, cut_ptr, Gp, Hp, 1.0f, reg, lo, hi, none.data(), unused);
          const GrowCand b = grow_node_split(G.data(), H.data(), F, cut_ptr, Gp, Hp, 1.0f, reg);
          EXPECT(a.valid == b.valid && a.key == b.key && same_bits(a.loss_chg, b.loss_chg) && a.GL == b.GL && a.HL == b.HL);
        }
      }
  }
}

int main() {
  check_policy();
  check_node_split();
  printf("grow_mono_host_check: %ld sums, %ld nodes, %ld failures\n", sums, nodes, failures);
  return failures == 0 ? 0 : 1;
}
