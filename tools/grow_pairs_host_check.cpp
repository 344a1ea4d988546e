// The host side of the boosting objectives (csrc/grow.hpp grow_pair, grow_pair_plane_bytes; grow.cpp plan_grow_weighted and
// the Deep plans) in a program of its own, for a build with -fsanitize=address,undefined (CPU only;
// tests/test_grow_objective_cpu.py builds and runs it): the pair planes in the plan over 1 to 2^31 rows, and the pair of
// both objectives over the edges of its domain - residuals from 0 and denormals to just below 256, weights from 0 to just
// below 256, every slope bound, and every input the pair refuses - written into planes of exactly n entries.
// Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_pairs_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static long plans = 0, pairs = 0;

static void check_plan(uint64_t n, uint32_t F, int depth, int cus) {
  ++plans;
  const uint64_t ncuts = (uint64_t)F * kGrowMaxCuts;
  const int top = std::min(depth, kGrowMaxDepth);
  const GrowPlan w = plan_grow_weighted(n, F, ncuts, top, cus);
  EXPECT(w.pairs_bytes == n * 12 && w.pairs_bytes == grow_pair_plane_bytes(n) && kGrowPairRowBytes == 12);
  EXPECT(w.pairs_bytes / kGrowPairRowBytes == n);                      // what the planes are allocated by
  EXPECT(plan_grow(n, F, ncuts, top, cus).pairs_bytes == 0);           // the count kind has no pair path
  const GrowDeepPlan d = plan_grow_deep(n, F, ncuts, depth, cus);
  EXPECT(d.lds.pairs_bytes == w.pairs_bytes);
  for (uint32_t n_sel : {1u, (F + 1) / 2, F}) {
    const GrowDeepPlan s = plan_grow_deep_sampled(n, F, n_sel, ncuts, depth, cus);
    EXPECT(s.lds.pairs_bytes == w.pairs_bytes);                        // every row has a pair, whatever a tree sees
  }
}

static void check_pairs() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float below = std::nextafterf(256.0f, 0.0f);
  const float zs[] = {0.0f, -0.0f, 0x1p-149f, -0x1p-149f, 0x1p-130f, 0x1p-126f, 0x1p-70f, -0x1p-70f, 1e-3f, 0.5f, -1.0f,
                      3.7f, 100.0f, -200.0f, below, -below, 256.0f, -256.0f, 1e30f, inf, -inf, nan};
  const float ws[] = {0.0f, 0x1p-24f, 0x1p-25f, 0.5f, 1.0f, 255.99f, below, 256.0f, -0.0f, -1.0f, inf, nan};
  const float slopes[] = {kGrowMinSlope, 0.5f, 1.0f, 3.7f, kGrowMaxSlope};
  const size_t n = sizeof zs / sizeof zs[0];
  for (uint32_t obj : {kGrowObjSquared, kGrowObjPseudoHuber})
    for (float slope : slopes)
      for (float w : ws) {
        std::vector<int64_t> q(n, 77);     // exactly n entries: a write past them is the sanitizer's to find
        std::vector<uint32_t> hq(n, 77);
        for (size_t r = 0; r < n; ++r) {
          ++pairs;
          // pred - label == z exactly: the label is 0
          const uint32_t flags = grow_pair_of(obj, slope, zs[r], 0.0f, w, &q[r], &hq[r]);
          const bool z_sound = std::fabs(zs[r]) < 256.0f, w_sound = w >= 0.0f && w < 256.0f;
          if (!z_sound) EXPECT(flags == kGrowFlagLabel && q[r] == 0 && hq[r] == 0);
          else if (!w_sound) EXPECT(flags == kGrowFlagWeight && q[r] == 0 && hq[r] == 0);
          else {
            EXPECT(flags == 0 || flags == kGrowFlagLabel);             // (|gw| >= 256 under a weight above 1)
            if (flags) EXPECT(q[r] == 0 && hq[r] == 0);
            EXPECT(q[r] > -(1ll << 32) && q[r] < (1ll << 32));
            if (flags == 0 && obj == kGrowObjSquared) EXPECT(hq[r] == (uint32_t)std::rint((double)w * 16777216.0));
            if (flags == 0 && zs[r] == 0.0f) EXPECT(q[r] == 0);
            if (flags == 0 && w == 0.0f) EXPECT(q[r] == 0 && hq[r] == 0);
            // a denormal residual: g is denormal or zero, and q is 0 whether or not denormals are flushed
            if (flags == 0 && std::fabs(zs[r]) < 0x1p-126f) EXPECT(q[r] == 0);
          }
        }
      }
  // the hessian of a far residual rounds to 0 at the smallest slope, and the gradient does not
  int64_t q;
  uint32_t hq;
  EXPECT(grow_pair_of(kGrowObjPseudoHuber, kGrowMinSlope, 200.5f, 0.0f, 1.0f, &q, &hq) == 0 && hq == 0 && q != 0);
  EXPECT(!grow_slope_sound(0.0f) && !grow_slope_sound(std::nextafterf(kGrowMinSlope, 0.0f)) && grow_slope_sound(kGrowMinSlope) &&
         grow_slope_sound(256.0f) && !grow_slope_sound(257.0f) && !grow_slope_sound(nan) && !grow_slope_sound(inf));
}

int main() {
  const uint64_t rows[] = {1, 2, 63, 64, 65, 255, 256, 257, 4097, 1ull << 20, 55987200ull, (1ull << 31) - 1, 1ull << 31};
  const uint32_t feats[] = {1, 3, 27, 128};
  for (uint64_t n : rows)
    for (uint32_t F : feats)
      for (int depth = 1; depth <= kGrowDeepMaxDepth; ++depth) check_plan(n, F, depth, n % 2 ? 256 : 1);
  check_plan(4097, 27, 18, 0);
  check_pairs();
  printf("grow_pairs_host_check: %ld plans, %ld pairs, %ld failures\n", plans, pairs, failures);
  return failures == 0 ? 0 : 1;
}
