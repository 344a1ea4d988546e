// Boosting new trees (include/ohxgb.h OHXBoosterBoostTrees; design in docs/18_boost_trees.md): `rounds` depth-limited
// regression trees are fitted, level by level, to the squared-error gradient of the caller's rows and labels and
// appended to the forest.  The rows are binned once against the caller's cuts (uint8, feature-major planes); a level's
// gradient histograms are integer sums kept in LDS and flushed with 64-bit global adds; a split is chosen from the
// histograms by a total order (largest loss_chg, then the smallest (feature, cut, default-left)), so that the result
// depends on neither the order of the rows nor the launch shape.  The gradient is the refit's 2^-24 fixed point and the
// leaf solve is refit_solve_leaf itself (refit.hpp).
//
// What host and device share is in this header: the gain, the comparison of two candidates, the hessian policy of the
// two kinds of hessian sum, the (gradient, hessian) pair of a row by the call's objective, the scan of one feature's bins
// over a policy, and the launch plan.  What the kernel files share is in grow_device.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <vector>

#include "refit.hpp"

#define OHX_GROW_HD OHX_REFIT_HD

namespace ohx {

constexpr uint32_t kGrowBins = 256;            // bins per (node, feature): 0 .. ncut, and the missing bin
constexpr uint32_t kGrowMissingBin = 255;
constexpr uint32_t kGrowMaxCuts = 254;         // per feature
constexpr uint32_t kGrowMaxFeatures = 128;     // the cuts of all features fit LDS: 128 x 254 floats
constexpr int kGrowMaxDepth = 8;
constexpr uint32_t kGrowMaxNodes = 512;        // node records kept per tree (a tree of depth 8 has at most 511)
// the Deep call (grow_deep.hip; design in docs/23_deep_trees.md): levels 8 and deeper keep their histograms in HBM
constexpr int kGrowDeepMaxDepth = 18;          // the depth the walk kernels, the path tables and the formats are exercised at
constexpr uint32_t kGrowDeepBatch = 1024;      // node slots whose histograms a batch of a deep level holds
constexpr uint32_t kGrowFlagLabel = 1u;        // the error word: a gradient out of range (refit.hpp kRefitFlagLabel)
constexpr uint32_t kGrowFlagState = 2u;        // a node id or a bin outside its table (never, from sound buffers)
constexpr uint32_t kGrowFlagEvalLabel = 4u;    // the same as kGrowFlagLabel at a held-out row
constexpr uint32_t kGrowFlagWeight = 8u;       // a training row's weight that is not finite, negative or >= 256
constexpr uint32_t kGrowFlagEvalWeight = 16u;  // the same at a held-out row
constexpr uint32_t kGrowFlagBag = 32u;         // a round whose bag of rows holds no weight (root H == 0)
constexpr uint32_t kGrowFlagHess = 64u;        // pseudo-Huber: a round whose root holds no hessian (root H == 0)

// gain(G, Hd) of the header: CalcGain of xgboost 1.6.0 with reg_alpha = 0 and max_delta_step = 0, on the fixed-point
// gradient sum and the hessian sum as its policy (below) makes it a double
OHX_GROW_HD inline double grow_gain(int64_t G, double Hd, double lambda) {
  const double Gd = (double)G * (1.0 / 16777216.0);
  return (Gd * Gd) / (Hd + lambda);
}

// One candidate.  key orders the candidates of a node: (feature << 9) | (j << 1) | dl
struct GrowCand {
  double loss_chg = 0.0;
  int64_t GL = 0;
  uint64_t HL = 0;
  uint32_t key = 0;
  uint32_t valid = 0;
};
OHX_GROW_HD inline uint32_t grow_key(uint32_t f, uint32_t j, uint32_t dl) { return (f << 9) | (j << 1) | dl; }

// The header's total order: a is taken over b when it is valid and b is not, when its loss_chg is larger (compared as
// doubles), or when they are equal and its key is smaller.  Associative and commutative as a reduction: the winner does
// not depend on who arrives first.
OHX_GROW_HD inline bool grow_better(const GrowCand& a, const GrowCand& b) {
  if (!a.valid) return false;
  if (!b.valid) return true;
  if (a.loss_chg > b.loss_chg) return true;
  if (a.loss_chg < b.loss_chg) return false;
  return a.key < b.key;
}

// ---- the hessian policy: what the two kinds of hessian sum do differently, for host and device alike ----

// A weight w is finite with 0 <= w < 256; the hessian of its row is hq = (uint64) rint(w * 2^24) < 2^32, and a sum H of
// up to 2^31 of them stays below 2^63.  Hd = (double)H * 2^-24: the conversion rounds to nearest even, the scaling is
// exact.
constexpr float kGrowMaxWeight = 256.0f;
OHX_GROW_HD inline double grow_hess(uint64_t H) { return (double)H * (1.0 / 16777216.0); }
// (NaN fails both comparisons)
OHX_GROW_HD inline bool grow_weight_sound(float w) { return w >= 0.0f && w < kGrowMaxWeight; }
// A node with Hd < 2 * min_child_weight is a leaf without evaluation
OHX_GROW_HD inline bool grow_weight_splits(uint64_t Hp, double min_child_weight) {
  return !(grow_hess(Hp) < 2.0 * min_child_weight);
}
// refit_solve_leaf with the fixed-point hessian sum: base_weight = (float)(-Gd / (Hd + lambda)), leaf = base_weight * eta
OHX_GROW_HD inline void grow_solve_leaf_weighted(int64_t G, uint64_t H, float eta, float lambda, float* leaf, float* weight) {
  const float w = (float)(-((double)G * (1.0 / 16777216.0)) / (grow_hess(H) + (double)lambda));
  *weight = w;
  *leaf = w * eta;
}

// ---- the objective: a row's (gradient, hessian) pair in fixed point (design in docs/26_objectives.md) ----

// "ohx_objective": what a row's pair is made from.  squarederror is g = z, h = 1; pseudohuber is xgboost 1.6.0's
// PseudoHuberRegression::GetGradient with slope delta ("ohx_huber_slope").
// quantile (design in docs/32_quantile_objective.md) is the pinball loss at alpha ("ohx_quantile_alpha"), which rides in
// the slope's place: g = 1 - alpha where z >= 0, else -alpha; h = 1.  Its leaves are not Newton steps: grow_quantile.hpp.
constexpr uint32_t kGrowObjSquared = 0, kGrowObjPseudoHuber = 1, kGrowObjQuantile = 2;
// the value of "ohx_objective" that names it
inline const char* grow_objective_name(uint32_t objective) {
  return objective == kGrowObjPseudoHuber ? "pseudohuber" : objective == kGrowObjQuantile ? "quantile" : "squarederror";
}
constexpr float kGrowMinSlope = 0.0009765625f;   // 2^-10
constexpr float kGrowMaxSlope = 256.0f;
// (NaN fails both comparisons)
inline bool grow_slope_sound(float slope) { return slope >= kGrowMinSlope && slope <= kGrowMaxSlope; }
// Bytes of the pair planes of n rows: an int64 q and a uint32 hq a row
constexpr uint64_t kGrowPairRowBytes = 8 + 4;
inline uint64_t grow_pair_plane_bytes(uint64_t nrow) { return nrow * kGrowPairRowBytes; }

// The pair of one row, the header's definition operation by operation: every operation is float32 and rounds once
// (-ffp-contract=off: no fused multiply-add), the division and the square root are IEEE.  Returns the flags the row
// raises (kGrowFlagLabel, kGrowFlagWeight), and then the pair (0, 0).  With slope >= 2^-10 and |z| < 256 nothing
// overflows (z2 / d2 < 2^36), and the result does not depend on whether float32 denormals are flushed: 1 + z2 / d2
// and d2 + z2 absorb a denormal z2, and a denormal g gives q = 0 either way.
template <uint32_t OBJ>
OHX_GROW_HD inline uint32_t grow_pair(float slope, float pred, float label, float w, int64_t* q, uint32_t* hq) {
  *q = 0;
  *hq = 0;
  const float z = pred - label;
  // the residual before the weight (a NaN fails the comparison)
  if (!(__builtin_fabsf(z) < kRefitMaxAbsGrad)) return kGrowFlagLabel;
  if (!grow_weight_sound(w)) return kGrowFlagWeight;
  float g = z, h = 1.0f;
  if (OBJ == kGrowObjPseudoHuber) {
    const float d2 = slope * slope;
    const float z2 = z * z;
    const float s = sqrtf(1.0f + z2 / d2);
    g = z / s;
    const float c = d2 + z2;
    h = d2 / (c * s);
  }
  if (OBJ == kGrowObjQuantile) g = z >= 0.0f ? 1.0f - slope : -slope;   // slope is alpha here; no division, no square root
  const float gw = g * w;
  if (!(__builtin_fabsf(gw) < kRefitMaxAbsGrad)) return kGrowFlagLabel;
  const float hw = h * w;
  *q = (int64_t)__builtin_rintf(gw * kRefitGradScale);
  *hq = (uint32_t)(uint64_t)__builtin_rintf(hw * kRefitGradScale);   // h <= 1 and w < 256: below 2^32
  return 0;
}
// the same with the objective as a value (the host's callers)
inline uint32_t grow_pair_of(uint32_t objective, float slope, float pred, float label, float w, int64_t* q, uint32_t* hq) {
  return objective == kGrowObjPseudoHuber ? grow_pair<kGrowObjPseudoHuber>(slope, pred, label, w, q, hq)
         : objective == kGrowObjQuantile  ? grow_pair<kGrowObjQuantile>(slope, pred, label, w, q, hq)
                                          : grow_pair<kGrowObjSquared>(slope, pred, label, w, q, hq);
}

// "count": H counts rows (OHXBoosterBoostTrees, OHXBoosterBoostTreesEval).  Children hold min_child_rows rows each.
struct GrowCountHess {
  uint64_t min_child_rows;
  OHX_GROW_HD double hess(uint64_t H) const { return (double)H; }
  OHX_GROW_HD bool admits(uint64_t HL, uint64_t HR) const { return !(HL < min_child_rows || HR < min_child_rows); }
  OHX_GROW_HD bool evaluates(uint64_t) const { return true; }
  OHX_GROW_HD float sum_hess(uint64_t H) const { return (float)H; }
  OHX_GROW_HD double gain(int64_t G, uint64_t H, double lambda) const { return grow_gain(G, hess(H), lambda); }
  OHX_GROW_HD void solve_leaf(int64_t G, uint64_t H, float eta, float lambda, float* leaf, float* weight) const {
    refit_solve_leaf(G, H, eta, lambda, leaf, weight);
  }
};
// "fixed-point": H sums hq (the calls with row weights).  Both children hold weight as integers (HL > 0 and HR > 0: no
// gain is taken of an empty child, so lambda == 0 divides by no zero) and both have Hd >= min_child_weight.
struct GrowFixedHess {
  double min_child_weight;
  OHX_GROW_HD double hess(uint64_t H) const { return grow_hess(H); }
  OHX_GROW_HD bool admits(uint64_t HL, uint64_t HR) const {
    if (HL == 0 || HR == 0) return false;
    return !(grow_hess(HL) < min_child_weight || grow_hess(HR) < min_child_weight);
  }
  OHX_GROW_HD bool evaluates(uint64_t Hp) const { return grow_weight_splits(Hp, min_child_weight); }
  OHX_GROW_HD float sum_hess(uint64_t H) const { return (float)grow_hess(H); }
  OHX_GROW_HD double gain(int64_t G, uint64_t H, double lambda) const { return grow_gain(G, hess(H), lambda); }
  OHX_GROW_HD void solve_leaf(int64_t G, uint64_t H, float eta, float lambda, float* leaf, float* weight) const {
    grow_solve_leaf_weighted(G, H, eta, lambda, leaf, weight);
  }
};

// ---- reg_alpha and max_delta_step (design in docs/27_regularisation_and_metrics.md) ----

// ThresholdL1 of xgboost 1.6.0's param.h on the gradient sum as a double: +0.0 where |Gd| <= alpha
OHX_GROW_HD inline double grow_threshold_l1(double Gd, double alpha) {
  return Gd > alpha ? Gd - alpha : (Gd < -alpha ? Gd + alpha : 0.0);
}
// The header's w of a node with D = Hd + lambda: (-T) / D, clipped to +-m where m > 0.  Every operation is a double
// operation and rounds once.  T == +0.0 gives -0.0 (D > 0).
OHX_GROW_HD inline double grow_reg_weight(double Gd, double D, double alpha, double m) {
  double w = (-grow_threshold_l1(Gd, alpha)) / D;
  if (m > 0.0 && __builtin_fabs(w) > m) w = __builtin_copysign(m, w);
  return w;
}
// The header's gain(G, H): T^2 / D where nothing can be clipped (m == 0), else twice the reduction of the regularised
// objective at the clipped w.  With alpha == 0 and m == 0 it is grow_gain bit for bit (Gd - 0.0 is Gd, and G == 0 gives
// 0.0 * 0.0 either way).
OHX_GROW_HD inline double grow_reg_gain(int64_t G, double Hd, double lambda, double alpha, double m) {
  const double Gd = (double)G * (1.0 / 16777216.0);
  const double D = Hd + lambda;
  if (m == 0.0) {
    const double T = grow_threshold_l1(Gd, alpha);
    return (T * T) / D;
  }
  const double w = grow_reg_weight(Gd, D, alpha, m);
  return -((2.0 * Gd) * w + (D * w) * w) - (2.0 * alpha) * __builtin_fabs(w);
}
// base_weight = (float)w, leaf = base_weight * eta (one float32 multiply).  With alpha == 0 and m == 0 it is
// grow_solve_leaf_weighted bit for bit, a base_weight of -0.0f at G == 0 included.
OHX_GROW_HD inline void grow_solve_leaf_reg(int64_t G, uint64_t H, float eta, float lambda, float alpha, float max_delta_step,
                                            float* leaf, float* weight) {
  const float w = (float)grow_reg_weight((double)G * (1.0 / 16777216.0), grow_hess(H) + (double)lambda, (double)alpha,
                                         (double)max_delta_step);
  *weight = w;
  *leaf = w * eta;
}
// (NaN fails both comparisons)
inline bool grow_reg_sound(float v) { return v >= 0.0f && v < INFINITY; }
// "regularised": GrowFixedHess with "ohx_reg_alpha" and "ohx_max_delta_step" in the gain and the leaf.  What a split may
// be (admits), which nodes are looked at (evaluates) and sum_hess are GrowFixedHess's.  16 bytes: a kernel argument.
struct GrowRegHess {
  double min_child_weight;
  float alpha, max_delta_step;
  OHX_GROW_HD double hess(uint64_t H) const { return grow_hess(H); }
  OHX_GROW_HD bool admits(uint64_t HL, uint64_t HR) const { return GrowFixedHess{min_child_weight}.admits(HL, HR); }
  OHX_GROW_HD bool evaluates(uint64_t Hp) const { return grow_weight_splits(Hp, min_child_weight); }
  OHX_GROW_HD float sum_hess(uint64_t H) const { return (float)grow_hess(H); }
  OHX_GROW_HD double gain(int64_t G, uint64_t H, double lambda) const {
    return grow_reg_gain(G, grow_hess(H), lambda, (double)alpha, (double)max_delta_step);
  }
  OHX_GROW_HD void solve_leaf(int64_t G, uint64_t H, float eta, float lambda, float* leaf, float* weight) const {
    grow_solve_leaf_reg(G, H, eta, lambda, alpha, max_delta_step, leaf, weight);
  }
};

// ---- monotone constraints (design in docs/28_monotone_constraints.md) ----

// "ohx_monotone_constraints": entry f is c_f in {-1, 0, +1}; at most one a feature
constexpr uint32_t kGrowMaxConstraints = kGrowMaxFeatures;
// The header's w(G, H; lo, hi): grow_reg_weight clamped into the node's interval.  -0.0 passes an interval that starts at
// +0.0 (it is not below it).
OHX_GROW_HD inline double grow_mono_weight(double Gd, double D, double alpha, double m, double lo, double hi) {
  const double w = grow_reg_weight(Gd, D, alpha, m);
  return w < lo ? lo : (w > hi ? hi : w);
}
// The header's gain_w(G, H, w): twice the reduction of the regularised objective at the weight w, the second form of
// grow_reg_gain at a weight that is given
OHX_GROW_HD inline double grow_gain_at(double Gd, double D, double alpha, double w) {
  return -((2.0 * Gd) * w + (D * w) * w) - (2.0 * alpha) * __builtin_fabs(w);
}
// "constrained": GrowRegHess as one (node, feature) sees it - with the node's interval (lo, hi) of weights and the
// feature's constraint c.  Its gain is gain_w at the clamped weight whatever max_delta_step is, and it admits a candidate
// by the gradient sums of both children too (its own grow_best_split below): the children's weights must stand in the order c asks
// for.  What GrowFixedHess admits, which nodes are looked at and sum_hess are unchanged.
struct GrowMonoHess {
  GrowRegHess reg;
  double lo, hi;
  int32_t c;
  OHX_GROW_HD double hess(uint64_t H) const { return grow_hess(H); }
  OHX_GROW_HD bool admits(uint64_t HL, uint64_t HR) const { return reg.admits(HL, HR); }
  OHX_GROW_HD bool evaluates(uint64_t Hp) const { return reg.evaluates(Hp); }
  OHX_GROW_HD float sum_hess(uint64_t H) const { return reg.sum_hess(H); }
  OHX_GROW_HD double weight(int64_t G, uint64_t H, double lambda) const {
    return grow_mono_weight((double)G * (1.0 / 16777216.0), grow_hess(H) + lambda, (double)reg.alpha, (double)reg.max_delta_step, lo,
                            hi);
  }
  OHX_GROW_HD double gain(int64_t G, uint64_t H, double lambda) const {
    return grow_gain_at((double)G * (1.0 / 16777216.0), grow_hess(H) + lambda, (double)reg.alpha, weight(G, H, lambda));
  }
  OHX_GROW_HD bool ordered(double wL, double wR) const { return c == 0 || (c > 0 ? wL <= wR : wL >= wR); }
  OHX_GROW_HD void solve_leaf(int64_t G, uint64_t H, float eta, float lambda, float* leaf, float* w) const {
    *w = (float)weight(G, H, (double)lambda);
    *leaf = *w * eta;
  }
  // The intervals of the children of a split on this policy's feature, out = (lo_L, hi_L, lo_R, hi_R): the parent's cut
  // at mid = (wL + wR) * 0.5 on the side c names, or the parent's own where c == 0
  OHX_GROW_HD void children(int64_t GL, uint64_t HL, int64_t GR, uint64_t HR, double lambda, double out[4]) const {
    out[0] = out[2] = lo;
    out[1] = out[3] = hi;
    if (c == 0) return;
    const double mid = (weight(GL, HL, lambda) + weight(GR, HR, lambda)) * 0.5;
    if (c > 0) out[1] = out[2] = mid;
    else out[0] = out[3] = mid;
  }
};
// What a split kernel of constrained boosting takes: the regularisation, the intervals of the tree at hand - two doubles
// (lo, hi) a node id; the root's is (-inf, +inf) and is never read, so nothing is reset between trees: every other node
// has its interval written when its parent splits - and the constraints of all num_feature features
struct GrowMonoArgs {
  GrowRegHess reg;
  double* bounds;
  const int8_t* constraints;
  OHX_GROW_HD GrowMonoHess at(uint32_t node, uint32_t f) const {
    GrowMonoHess h;
    h.reg = reg;
    h.lo = node == 0 ? -INFINITY : bounds[2 * (uint64_t)node];
    h.hi = node == 0 ? INFINITY : bounds[2 * (uint64_t)node + 1];
    h.c = constraints[f];
    return h;
  }
};

// The best candidate among cuts j0 .. j0 + n - 1 (those below ncut) of feature f.  G / H point at bin j0; GLb / HLb
// are the sums over the bins below j0; Gm / Hm the missing bin; Gp / Hp the node.  Candidates are visited in ascending
// (j, dl) and replaced only by a strictly better one.  The host calls it with j0 = 0, n = ncut; a lane of a split
// kernel with its four bins.
template <class Hess>
OHX_GROW_HD inline GrowCand grow_best_split(const int64_t* G, const uint64_t* H, uint32_t f, uint32_t j0, uint32_t n,
                                            uint32_t ncut, int64_t GLb, uint64_t HLb, int64_t Gm, uint64_t Hm, int64_t Gp,
                                            uint64_t Hp, double lambda, const Hess& hess) {
  GrowCand best;
  const double parent = hess.gain(Gp, Hp, lambda);
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t j = j0 + k;
    GLb += G[k];
    HLb += H[k];
    if (j >= ncut) continue;
    for (uint32_t dl = 0; dl < 2; ++dl) {
      GrowCand c;
      c.GL = dl ? GLb + Gm : GLb;
      c.HL = dl ? HLb + Hm : HLb;
      const int64_t GR = Gp - c.GL;
      const uint64_t HR = Hp - c.HL;
      if (!hess.admits(c.HL, HR)) continue;
      c.loss_chg = (hess.gain(c.GL, c.HL, lambda) + hess.gain(GR, HR, lambda)) - parent;
      c.key = grow_key(f, j, dl);
      c.valid = 1;
      if (grow_better(c, best)) best = c;
    }
  }
  return best;
}

// The same scan for the constrained policy, written beside the one above so that no other instantiation moves: a
// candidate is admitted by the hessian sums as ever and by the order of the children's weights, and its loss_chg is taken
// at those weights.  The candidates, their order and the ties are the scan's above.
template <>
OHX_GROW_HD inline GrowCand grow_best_split<GrowMonoHess>(const int64_t* G, const uint64_t* H, uint32_t f, uint32_t j0, uint32_t n,
                                                          uint32_t ncut, int64_t GLb, uint64_t HLb, int64_t Gm, uint64_t Hm,
                                                          int64_t Gp, uint64_t Hp, double lambda, const GrowMonoHess& hess) {
  GrowCand best;
  const double alpha = (double)hess.reg.alpha;
  const double parent = hess.gain(Gp, Hp, lambda);
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t j = j0 + k;
    GLb += G[k];
    HLb += H[k];
    if (j >= ncut) continue;
    for (uint32_t dl = 0; dl < 2; ++dl) {
      GrowCand c;
      c.GL = dl ? GLb + Gm : GLb;
      c.HL = dl ? HLb + Hm : HLb;
      const int64_t GR = Gp - c.GL;
      const uint64_t HR = Hp - c.HL;
      if (!hess.admits(c.HL, HR)) continue;
      const double wL = hess.weight(c.GL, c.HL, lambda), wR = hess.weight(GR, HR, lambda);
      if (!hess.ordered(wL, wR)) continue;
      c.loss_chg = (grow_gain_at((double)c.GL * (1.0 / 16777216.0), grow_hess(c.HL) + lambda, alpha, wL) +
                    grow_gain_at((double)GR * (1.0 / 16777216.0), grow_hess(HR) + lambda, alpha, wR)) -
                   parent;
      c.key = grow_key(f, j, dl);
      c.valid = 1;
      if (grow_better(c, best)) best = c;
    }
  }
  return best;
}

// ---- row and column subsampling (OHXBoosterBoostTreesSampled; design in docs/22_sampling.md) ----

// The header's mix function; all arithmetic is uint64 and wraps.
constexpr uint64_t kGrowGamma64 = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kGrowSampleOne = 1u << 24;   // k_s of subsample 1.0f: every row is in and nothing is drawn
OHX_GROW_HD inline uint64_t grow_mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// K_row(i) and K_col(i) of tree i, counted over the whole forest
OHX_GROW_HD inline uint64_t grow_row_key(uint64_t seed, uint64_t i) { return grow_mix(seed + kGrowGamma64 * (2ull * i + 1ull)); }
OHX_GROW_HD inline uint64_t grow_col_key(uint64_t seed, uint64_t i) { return grow_mix(seed + kGrowGamma64 * (2ull * i + 2ull)); }
// row r is in the bag of the tree with key K_row when the top 24 bits of its draw lie below k_s
OHX_GROW_HD inline bool grow_in_bag(uint64_t row_key, uint64_t r, uint32_t k_s) { return (uint32_t)(grow_mix(row_key + r) >> 40) < k_s; }
// k_s = (uint32) rint((double)subsample * 2^24); 0 where subsample is not finite, <= 0 or > 1 (0 is refused)
inline uint32_t grow_sample_threshold(float subsample) {
  if (!(subsample > 0.0f && subsample <= 1.0f)) return 0;
  return (uint32_t)std::rint((double)subsample * 16777216.0);
}
// n_sel = max(1, (int) floor((double)colsample * F)); 0 where colsample is not finite, <= 0 or > 1
inline uint32_t grow_num_selected(uint32_t F, float colsample) {
  if (!(colsample > 0.0f && colsample <= 1.0f) || F == 0) return 0;
  const uint32_t n = (uint32_t)std::floor((double)colsample * (double)F);
  return n < 1 ? 1 : n;
}

// ---- column sampling by level and by node ("ohx_colsample_bylevel", "ohx_colsample_bynode"; design in
// docs/29_colsample_level_node.md) ----

// K_lvl(i, d) and K_node(i, p) from K_col(i): d is the depth of the nodes being split (the root's is 0), p the node's id
// in the tree in allocation order.  d + 1 <= 18 < 32, so a level key and a node key never share an input.
constexpr uint64_t kGrowNodeKeyBase = 32;
OHX_GROW_HD inline uint64_t grow_level_key(uint64_t col_key, uint32_t d) { return grow_mix(col_key + kGrowGamma64 * ((uint64_t)d + 1ull)); }
OHX_GROW_HD inline uint64_t grow_node_key(uint64_t col_key, uint32_t p) {
  return grow_mix(col_key + kGrowGamma64 * (kGrowNodeKeyBase + (uint64_t)p));
}
// (key, f) of one feature below that of another: the order both draws take their smallest by
OHX_GROW_HD inline bool grow_draw_below(uint64_t ka, uint32_t fa, uint64_t kb, uint32_t fb) { return ka != kb ? ka < kb : fa < fb; }
// What a split kernel of a column-sampled call takes: the lists of every round and level of the call, [rounds][depth][n_lvl]
// bytes on the device, each ascending; n_node of the n_lvl features of its level are a node's; and what K_col of round r is
// made from, the tree being tree0 + r of the draws.
struct GrowColsampleArgs {
  const uint8_t* lists = nullptr;
  uint32_t depth = 0, n_lvl = 0, n_node = 0;
  uint64_t seed = 0, tree0 = 0;
  OHX_GROW_HD const uint8_t* list(uint32_t round, uint32_t level) const {
    return lists + ((uint64_t)round * depth + level) * n_lvl;
  }
  OHX_GROW_HD uint64_t col_key(uint32_t round) const { return grow_col_key(seed, tree0 + round); }
};

// ---- interaction constraints ("ohx_interaction_constraints"; design in docs/35_interaction_constraints.md) ----

// A set of feature ids is two uint64 words, bit f % 64 of word f / 64.  The groups are ngroups x 2 words.
constexpr uint32_t kGrowMaxGroups = 64;
static_assert(kGrowMaxFeatures == 128, "a set of features is two 64-bit words");
OHX_GROW_HD inline bool grow_interact_has(const uint64_t set[2], uint32_t f) {
  return f < kGrowMaxFeatures && (((f < 64 ? set[0] : set[1]) >> (f & 63u)) & 1ull) != 0;
}
// every feature 0 .. F - 1 (F <= 128)
OHX_GROW_HD inline void grow_interact_all(uint32_t F, uint64_t out[2]) {
  out[0] = F >= 64 ? ~0ull : (1ull << F) - 1ull;
  out[1] = F >= 128 ? ~0ull : (F > 64 ? (1ull << (F - 64)) - 1ull : 0ull);
}
// The header's A of a node whose path has split on the features P: every feature 0 .. F - 1 where P is empty (the root),
// else P and every group that holds all of P.  The one function the host and the split kernels use.
OHX_GROW_HD inline void grow_interact_allowed(const uint64_t P[2], const uint64_t* groups, uint32_t ngroups, uint32_t F, uint64_t out[2]) {
  if ((P[0] | P[1]) == 0) {
    grow_interact_all(F, out);
    return;
  }
  uint64_t a0 = P[0], a1 = P[1];
  for (uint32_t g = 0; g < ngroups; ++g) {
    const uint64_t g0 = groups[2 * g], g1 = groups[2 * g + 1];
    if ((P[0] & ~g0) == 0 && (P[1] & ~g1) == 0) {
      a0 |= g0;
      a1 |= g1;
    }
  }
  out[0] = a0;
  out[1] = a1;
}
// The value of "ohx_interaction_constraints" by the header's grammar: the groups' words into `words` (ngroups x 2) and
// true, or false, and `words` as it was.
bool grow_interact_parse(const char* value, std::vector<uint64_t>* words);
// Whether the groups take a candidate away from some node of a booster with F features: false for no group, and where a
// group holds every feature 0 .. F - 1.
bool grow_interact_active(const uint64_t* groups, uint32_t ngroups, uint32_t F);
// What a split kernel of a call under interaction constraints takes: the groups, the sets of the tree at hand - four words
// a node id, P then A; the root's are ({}, every feature) and are never read, so nothing is reset between trees: every
// other node has its sets written when its parent splits - and the policy the call has underneath (GrowFixedHess,
// GrowRegHess or GrowMonoArgs), whose gain, leaf solve and records are unchanged.
template <class Policy>
struct GrowInteractArgs {
  const uint64_t* groups;
  uint64_t* sets;
  uint32_t ngroups;
  Policy inner;
};

// A node as the device leaves it.  Children are written as leaves when their parent splits and overwritten if they
// split in turn, so every record is complete whenever the level loop stops.
struct GrowNode {
  int64_t G;            // the node's sums
  uint64_t H;
  int32_t left, right;  // -1: a leaf
  int32_t parent;       // the file's form: bit 31 = left child, root = -1
  uint32_t feature;
  uint32_t cut;         // j of the split (device only: the partition compares bins with it)
  uint32_t default_left;
  float value;          // c_j, or the leaf value
  float loss_chg, sum_hess, base_weight;
};

// ---- the host side (grow.cpp) ----

// OHXQuantileCuts of the header.  Returns the number of cut values needed; writes cut_ptr (ncol + 1) always and
// cut_values when they fit `cap`.
uint64_t quantile_cuts(const float* data, uint64_t nrow, uint64_t ncol, float missing, int max_bins, uint64_t* cut_ptr,
                       float* cut_values, uint64_t cap);
// Throws OhxError(what + ...) unless cut_ptr starts at 0, ascends, holds at most 254 cuts per feature, and the values
// are finite and strictly ascending within a feature.
void grow_check_cuts(const uint64_t* cut_ptr, const float* cut_values, uint32_t num_feature, const char* what);
// The best split of one node over all features from its histograms G / H [num_feature][256] (grow_best_split per
// feature, ascending, replaced by a strictly better one only).  A node its policy does not evaluate has no candidate.
template <class Hess>
inline GrowCand grow_node_split(const int64_t* G, const uint64_t* H, uint32_t num_feature, const uint64_t* cut_ptr, int64_t Gp,
                                uint64_t Hp, float lambda, const Hess& hess) {
  GrowCand best;
  if (!hess.evaluates(Hp)) return best;
  for (uint32_t f = 0; f < num_feature; ++f) {
    const int64_t* g = G + (size_t)f * kGrowBins;
    const uint64_t* h = H + (size_t)f * kGrowBins;
    const uint32_t ncut = (uint32_t)(cut_ptr[f + 1] - cut_ptr[f]);
    const GrowCand c = grow_best_split(g, h, f, 0, ncut, ncut, 0, 0, g[kGrowMissingBin], h[kGrowMissingBin], Gp, Hp,
                                       (double)lambda, hess);
    if (grow_better(c, best)) best = c;
  }
  return best;
}
// The same under monotone constraints: the node's interval (lo, hi), and feature f scanned with constraints[f] (num_feature
// entries).  children: the intervals grow_write_split hands the children of the winner, (lo_L, hi_L, lo_R, hi_R).
inline GrowCand grow_mono_node_split(const int64_t* G, const uint64_t* H, uint32_t num_feature, const uint64_t* cut_ptr, int64_t Gp,
                                     uint64_t Hp, float lambda, const GrowRegHess& reg, double lo, double hi, const int8_t* constraints,
                                     double children[4]) {
  GrowCand best;
  GrowMonoHess hess{reg, lo, hi, 0};
  hess.children(0, 0, 0, 0, (double)lambda, children);
  if (!hess.evaluates(Hp)) return best;
  for (uint32_t f = 0; f < num_feature; ++f) {
    const int64_t* g = G + (size_t)f * kGrowBins;
    const uint64_t* h = H + (size_t)f * kGrowBins;
    const uint32_t ncut = (uint32_t)(cut_ptr[f + 1] - cut_ptr[f]);
    hess.c = constraints[f];
    const GrowCand c = grow_best_split(g, h, f, 0, ncut, ncut, 0, 0, g[kGrowMissingBin], h[kGrowMissingBin], Gp, Hp, (double)lambda, hess);
    if (grow_better(c, best)) best = c;
  }
  if (best.valid) {
    hess.c = constraints[best.key >> 9];
    hess.children(best.GL, best.HL, Gp - best.GL, Hp - best.HL, (double)lambda, children);
  }
  return best;
}
// The features of tree i: the n_sel = grow_num_selected(F, colsample) features smallest by (mix(K_col(i) + f), f), written
// to out[0 .. n_sel) in ascending f.  n_sel == F writes 0 .. F - 1 and draws nothing.  Returns n_sel (0: colsample is
// unsound, F is 0 or above kGrowMaxFeatures; nothing is written).
uint32_t grow_pick_features(uint64_t seed, uint64_t i, uint32_t F, float colsample, uint8_t* out);
// The features of level d of tree i: the n_lvl = grow_num_selected(n_sel, bylevel) features of tree_list[0 .. n_sel)
// smallest by (mix(K_lvl(i, d) + f), f), written to out[0 .. n_lvl) in the list's order.  n_lvl == n_sel copies the list
// and draws nothing.  Returns n_lvl (0: bylevel is unsound, n_sel is 0 or above kGrowMaxFeatures; nothing is written).
uint32_t grow_pick_level_features(uint64_t seed, uint64_t i, uint32_t d, const uint8_t* tree_list, uint32_t n_sel, float bylevel,
                                  uint8_t* out);
// The same for node p of that level over level_list[0 .. n_lvl): n_node = grow_num_selected(n_lvl, bynode) features by
// (mix(K_node(i, p) + f), f).
uint32_t grow_pick_node_features(uint64_t seed, uint64_t i, uint32_t p, const uint8_t* level_list, uint32_t n_lvl, float bynode,
                                 uint8_t* out);
// Whether f is one of them, as a split kernel finds it: the features of the level's list that lie below f by (key, f) are
// counted, and f is in where they are fewer than n_node.  n_node >= n_lvl counts nothing.  f must be in the list.
inline bool grow_node_has_feature(uint64_t seed, uint64_t i, uint32_t p, const uint8_t* level_list, uint32_t n_lvl, uint32_t n_node,
                                  uint32_t f) {
  if (n_node >= n_lvl) return true;
  const uint64_t key = grow_node_key(grow_col_key(seed, i), p);
  const uint64_t mine = grow_mix(key + f);
  uint32_t below = 0;
  for (uint32_t k = 0; k < n_lvl; ++k) below += grow_draw_below(grow_mix(key + level_list[k]), level_list[k], mine, f) ? 1u : 0u;
  return below < n_node;
}
// A Tree of the forest from n node records (at most max_nodes: the stride of the call's node table); throws on a record
// that is not a tree in allocation order.
Tree grow_assemble_tree(const GrowNode* nodes, uint32_t n, uint32_t num_feature, uint32_t max_nodes = kGrowMaxNodes);

// ---- the held-out metric (OHXBoosterBoostTreesEval; design in docs/20_boost_eval.md) ----

// A sum of squares S = sum q^2 as the device keeps it: `hi` sums the high 32 bits of each q^2 and `lo` the low 32
// bits, so S = hi * 2^32 + lo.  With at most 2^31 rows neither accumulator overflows.
struct GrowSum {
  uint64_t hi = 0, lo = 0;
};
// lo < 2^32 afterwards; what it held above goes into hi
inline GrowSum grow_sum_normal(GrowSum s) {
  GrowSum n;
  n.hi = s.hi + (s.lo >> 32);
  n.lo = s.lo & 0xFFFFFFFFull;
  return n;
}
// a < b as the exact integers
inline bool grow_sum_less(GrowSum a, GrowSum b) {
  a = grow_sum_normal(a);
  b = grow_sum_normal(b);
  return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo;
}
// the same where a sum is held as the exact integer itself (grow_sum_value)
inline bool grow_sum_less(unsigned __int128 a, unsigned __int128 b) { return a < b; }
// One step of the stop rule: the best round once S[t] is known.  Strict: a tie is not an improvement.
template <class Sum>
inline uint32_t grow_eval_best(const Sum* S, uint32_t best, uint32_t t) { return grow_sum_less(S[t], S[best]) ? t : best; }
inline bool grow_eval_stops(uint32_t best, uint32_t t, int patience) {
  return patience >= 1 && t - best >= (uint32_t)patience;
}
// The stop rule over the held-out sums S[0 .. rounds]: best starts at 0; after tree t, best = t if S[t] < S[best]; with
// patience >= 1 the run stops at the first t with t - best >= patience.  Sums past *rounds_run are not looked at.
template <class Sum>
inline void grow_eval_stop(const Sum* S, uint32_t rounds, int patience, uint32_t* rounds_run, uint32_t* best) {
  uint32_t b = 0, run = rounds;
  for (uint32_t t = 1; t <= rounds; ++t) {
    b = grow_eval_best(S, b, t);
    if (grow_eval_stops(b, t, patience)) {
      run = t;
      break;
    }
  }
  *rounds_run = run;
  *best = b;
}
// sqrt( (double)S * 2^-48 / (double)n ): the exact integer rounded to nearest even as it becomes a double, an exact
// scaling, then an IEEE division and square root.
double grow_sum_rmse(GrowSum s, uint64_t n);

// The weighted sum of squares S = sum hq * e^2 (e the unweighted fixed-point residual) as the device keeps it.  With
// e^2 = a * 2^32 + b (a, b < 2^32) a row adds (hq * a) >> 32 to p2, ((hq * a) & m) + ((hq * b) >> 32) to p1 and
// (hq * b) & m to p0, m = 0xFFFFFFFF: S = p2 * 2^64 + p1 * 2^32 + p0 < 2^127.  A row adds less than 2^32 to p2 and p0
// and at most 2^33 - 2 to p1: with at most 2^31 rows p2, p0 < 2^63 and p1 <= 2^64 - 2^32, so none overflows.
struct GrowWideSum {
  uint64_t p2 = 0, p1 = 0, p0 = 0;
};
inline unsigned __int128 grow_wide_value(GrowWideSum s) {
  return ((unsigned __int128)s.p2 << 64) + ((unsigned __int128)s.p1 << 32) + (unsigned __int128)s.p0;
}
// a < b as the exact integers (the stop rule's comparison: grow_eval_best and grow_eval_stop take either sum)
inline bool grow_sum_less(GrowWideSum a, GrowWideSum b) { return grow_wide_value(a) < grow_wide_value(b); }
// Either sum as the exact integer, from the device's words: (hi, lo) where words == 2, (p2, p1, p0) where words == 3.
// Each word stands 2^32 above the next.
inline unsigned __int128 grow_sum_value(const unsigned long long* s, size_t words) {
  unsigned __int128 v = 0;
  for (size_t k = 0; k < words; ++k) v = (v << 32) + (unsigned __int128)s[k];
  return v;
}
// sqrt( ((double)S * 2^-72) / ((double)W * 2^-24) ), W = sum hq: both exact integers rounded to nearest even as they
// become doubles, exact scalings, then an IEEE division and square root.
double grow_wide_rmse(GrowWideSum s, uint64_t W);

// "ohx_eval_metric": what one row adds to S beside its hq (design in docs/27_regularisation_and_metrics.md).  rmse is the
// square of the fixed-point residual, as ever; mae its size; pseudohuber delta^2 (sqrt(1 + z^2 / delta^2) - 1) in the
// form that cancels nothing, every operation float32 and rounding once, the division and the square root IEEE.
// quantile is the pinball loss at alpha (in the slope's place): the size of the fixed-point residual times alpha_q where
// z < 0 and 2^24 - alpha_q where not, below 2^56; its sums stand 2^24 above mae's (grow_wide_quantile).
constexpr uint32_t kGrowMetricRmse = 0, kGrowMetricMae = 1, kGrowMetricPseudoHuber = 2, kGrowMetricQuantile = 3;
// "ohx_quantile_alpha": 2^-10 <= alpha <= 1 - 2^-10 (NaN fails both comparisons), and alpha_q = rint(alpha * 2^24): the
// scaling of a float32 by 2^24 is exact, so 2^14 <= alpha_q <= 2^24 - 2^14
constexpr float kGrowMinAlpha = 0.0009765625f, kGrowMaxAlpha = 0.9990234375f;
inline bool grow_alpha_sound(float alpha) { return alpha >= kGrowMinAlpha && alpha <= kGrowMaxAlpha; }
OHX_GROW_HD inline uint32_t grow_alpha_q(float alpha) { return (uint32_t)__builtin_rintf(alpha * kRefitGradScale); }
// sq of the header for z = pred - label; false (and sq = 0) where z is not finite or |z| >= 256.  sq < 2^64 for rmse,
// < 2^32 for mae and < 2^40 for pseudohuber (mf <= delta |z| < 2^16).  A denormal z2 or mf gives 0 whether or not
// denormals are flushed: 1 + z2 / d2 absorbs the one and rint(mf * 2^24) the other.
template <uint32_t METRIC>
OHX_GROW_HD inline bool grow_metric_row(float slope, float pred, float label, uint64_t* sq) {
  *sq = 0;
  const float z = pred - label;
  // (a NaN fails the comparison)
  if (!(__builtin_fabsf(z) < kRefitMaxAbsGrad)) return false;
  if (METRIC == kGrowMetricPseudoHuber) {
    const float d2 = slope * slope;
    const float z2 = z * z;
    const float s = sqrtf(1.0f + z2 / d2);
    const float mf = z2 / (1.0f + s);
    *sq = (uint64_t)__builtin_rintf(mf * kRefitGradScale);
    return true;
  }
  const long long e = (long long)__builtin_rintf(z * kRefitGradScale);
  const uint64_t m = (uint64_t)(e < 0 ? -e : e);   // <= 2^32 - 256
  if (METRIC == kGrowMetricQuantile) {
    const uint32_t alpha_q = grow_alpha_q(slope);   // slope is alpha here
    *sq = m * (uint64_t)(z < 0.0f ? alpha_q : kGrowSampleOne - alpha_q);
    return true;
  }
  *sq = METRIC == kGrowMetricMae ? m : m * m;
  return true;
}
// the same with the metric as a value (the host's callers)
inline bool grow_metric_row_of(uint32_t metric, float slope, float pred, float label, uint64_t* sq) {
  return metric == kGrowMetricPseudoHuber ? grow_metric_row<kGrowMetricPseudoHuber>(slope, pred, label, sq)
         : metric == kGrowMetricMae       ? grow_metric_row<kGrowMetricMae>(slope, pred, label, sq)
         : metric == kGrowMetricQuantile  ? grow_metric_row<kGrowMetricQuantile>(slope, pred, label, sq)
                                          : grow_metric_row<kGrowMetricRmse>(slope, pred, label, sq);
}
// What mae and pseudohuber report: ((double)S * 2^-48) / ((double)W * 2^-24), both exact integers rounded to nearest
// even as they become doubles, exact scalings, then an IEEE division.  No square root.
double grow_wide_mean(GrowWideSum s, uint64_t W);
// What quantile reports: ((double)S * 2^-72) / ((double)W * 2^-24), likewise.  No square root.
double grow_wide_quantile(GrowWideSum s, uint64_t W);

// ---- the launch plan ----

constexpr uint32_t kGrowBlock = 256;           // bin, split, partition and leaf kernels: a row per lane
constexpr uint32_t kGrowHistBlock = 1024;      // the histogram kernel: sixteen waves share a block's LDS histogram
constexpr uint32_t kGrowRowBlocksPerCu = 8;    // the streaming kernels
constexpr uint32_t kGrowHistBlocksPerCu = 2;   // over all of gridDim.y
constexpr uint32_t kGrowLdsBytes = 160 * 1024; // a CU's LDS
constexpr uint32_t kGrowPairBytes = kGrowBins * (8 + 4);          // one (node, feature) histogram in LDS
constexpr uint32_t kGrowMaxPairs = kGrowLdsBytes / kGrowPairBytes; // 53
constexpr uint32_t kGrowWeightedPairBytes = kGrowBins * (8 + 8);                   // with a fixed-point hessian sum
constexpr uint32_t kGrowWeightedMaxPairs = kGrowLdsBytes / kGrowWeightedPairBytes; // 40
// a block's 32-bit LDS count of a bin cannot overflow: trips x 1024 rows stay below 2^32
constexpr uint64_t kGrowMaxTrips = (1ull << 22) - 1;

struct GrowLevelPlan {
  uint32_t slots = 0;         // node slots of the level: 2^d
  uint32_t node_group = 0;    // node slots per block
  uint32_t feat_group = 0;    // features per block
  uint32_t node_groups = 0, feat_groups = 0;   // gridDim.y = node_groups x feat_groups
  uint32_t hist_blocks = 0;   // gridDim.x: blocks over the rows
  uint32_t lds_bytes = 0;     // node_group x feat_group x 256 x 12 (x 16 in the weighted plan)
};
struct GrowPlan {
  uint32_t row_blocks = 0;    // bin, partition and leaf kernels; one trip is row_blocks x 256 rows
  uint32_t bin_lds_bytes = 0; // the staged cuts
  std::vector<GrowLevelPlan> levels;   // max_depth entries
  uint64_t bins_bytes = 0;    // num_feature x nrow
  uint64_t hist_bytes = 0;    // the deepest level's global histograms: slots x num_feature x 256 x 16
  uint64_t pairs_bytes = 0;   // the pair planes where the pair path runs (grow_pairs.hip): nrow x 12; 0 in plan_grow
};
GrowPlan plan_grow(uint64_t nrow, uint32_t num_feature, uint64_t ncuts, int max_depth, int num_cus);
// the same for grow_hist_weighted_kernel: 16 bytes a bin, at most 40 (node, feature) pairs a block
GrowPlan plan_grow_weighted(uint64_t nrow, uint32_t num_feature, uint64_t ncuts, int max_depth, int num_cus);
// blocks of grow_sse_kernel and grow_walk_sse_kernel over n rows: a row per lane, kGrowBlock lanes, grid-stride
uint32_t plan_grow_eval_blocks(uint64_t nrow, int num_cus);

// ---- the Deep call's plan ----

// Node records of one round: min(2^(max_depth + 1), 2 * nrow).  A split needs weight on both sides, so every leaf holds
// a row and a tree has at most 2 * nrow - 1 nodes; by its depth at most 2^(max_depth + 1) - 1.
inline uint64_t grow_deep_node_stride(uint64_t nrow, int max_depth) {
  return std::min<uint64_t>(1ull << (max_depth + 1), 2 * nrow);
}
// The open nodes a level can have at most: half a full last level's children, and never more than the rows.
inline uint64_t grow_deep_max_open(uint64_t nrow, int max_depth) {
  return std::max<uint64_t>(1, std::min<uint64_t>(1ull << (max_depth - 1), nrow));
}
struct GrowDeepPlan {
  GrowPlan lds;               // plan_grow_weighted over levels 0 .. min(max_depth, 8) - 1
  uint32_t batch = 0;         // kGrowDeepBatch
  uint32_t hist_blocks = 0;   // grid of grow_deep_hist_kernel: kGrowBlock lanes a block, a row per lane, grid-stride
  uint64_t scratch_bytes = 0; // Ghist and Hhist of one batch together: min(batch, max open) x F x 256 x 16; 0 at depth <= 8
  uint64_t best_bytes = 0;    // the candidates of a level: max(max open, 2^(min(max_depth, 8) - 1)) x F x sizeof(GrowCand)
  uint64_t node_stride = 0;   // grow_deep_node_stride
};
GrowDeepPlan plan_grow_deep(uint64_t nrow, uint32_t num_feature, uint64_t ncuts, int max_depth, int num_cus);
// The same for a tree that sees n_sel of the num_feature features (OHXBoosterBoostTreesDeepSampled): plan_grow_deep over
// n_sel histogram columns - lds is plan_grow_weighted(nrow, n_sel, ..), the scratch min(batch, max open) x n_sel x 256 x
// 16 bytes and `best` max(max open, 128) x n_sel candidates - with the bin planes of all num_feature features.
// n_sel == num_feature is plan_grow_deep itself.
GrowDeepPlan plan_grow_deep_sampled(uint64_t nrow, uint32_t num_feature, uint32_t n_sel, uint64_t ncuts, int max_depth, int num_cus);

// The child ids of a level with any number of open nodes, as one block of `width` lanes hands them out: the slots are
// walked in chunks of `width` with a running total; a slot's `below` is the running total plus the exclusive scan of
// its chunk's split flags, and its children are grow_child_id(next, below) and the id after it - so ids ascend in node
// order across chunk borders.  The host's statement, scanned serially; grow_deep_split_kernel scans a chunk with ballots
// and takes its ids from the same grow_child_id.  left[s] is written where flag[s] != 0.  Returns the splits.
OHX_GROW_HD inline uint32_t grow_child_id(uint32_t next, uint32_t below) { return next + 2u * below; }
inline uint32_t grow_chunked_children(const uint8_t* flag, uint32_t count, uint32_t width, uint32_t next, uint32_t* left) {
  uint32_t running = 0;
  for (uint32_t c0 = 0; c0 < count; c0 += width) {
    const uint32_t nc = count - c0 < width ? count - c0 : width;
    uint32_t scan = 0;
    for (uint32_t i = 0; i < nc; ++i) {
      if (flag[c0 + i]) left[c0 + i] = grow_child_id(next, running + scan);
      scan += flag[c0 + i] ? 1u : 0u;
    }
    running += scan;
  }
  return running;
}

#ifdef __HIPCC__
struct GrowLevelState {   // one per call, on the device
  uint32_t begin, end;    // the open nodes of the level at hand: ids [begin, end)
  uint32_t next;          // the next id to allocate = the tree's nodes so far
  uint32_t error;         // kGrowFlag*
};
struct GrowArgs {
  // the rows
  const float* rows = nullptr;     // [nrow][ncol]
  uint64_t nrow = 0;
  uint32_t ncol = 0, num_feature = 0;
  float missing = 0.0f;
  const float* labels = nullptr;   // [nrow]
  // the cuts
  const uint32_t* cut_ptr = nullptr;   // [num_feature + 1]
  const float* cuts = nullptr;
  uint32_t ncuts = 0;
  // the grower's own buffers
  uint8_t* bins = nullptr;         // [num_feature][nrow]
  uint16_t* pos = nullptr;         // [nrow] the node a row stands on
  float* pred = nullptr;           // [nrow] the margin of the forest so far
  unsigned long long* Ghist = nullptr;   // [slots][num_feature][256] int64 as two's complement
  unsigned long long* Hhist = nullptr;   // [slots][num_feature][256]
  GrowCand* best = nullptr;        // [slots][num_feature]
  GrowNode* nodes = nullptr;       // [rounds][kGrowMaxNodes]
  uint32_t* tree_nodes = nullptr;  // [rounds] nodes of each tree
  GrowLevelState* state = nullptr;
  int max_depth = 0;
  float eta = 0.0f, lambda = 0.0f, gamma = 0.0f;
  uint64_t min_child_rows = 1;
  // row weights (grow_weighted.hip, grow_sampled.hip): Hhist and GrowNode.H hold fixed-point hessian sums, and
  // min_child_rows is not read
  const float* weights = nullptr;      // [nrow], or nullptr: every weight is 1.0f
  double min_child_weight = 0.0;
  // row and column subsampling (grow_sampled.hip): the histograms, `best` and the memsets are compact,
  // [slots][n_sel][256]; the node records, pos, pred and the bins are those of every call
  unsigned long long* bag = nullptr;   // [ceil(nrow / 64)] a bit a row, or nullptr: every row is in the bag
  const uint8_t* features = nullptr;   // [rounds][n_sel] the selected features of every round, ascending
  uint32_t n_sel = 0;
  uint64_t row_key = 0;                // K_row of the tree at hand (grow_bag_kernel)
  uint32_t k_s = kGrowSampleOne;
};
// Once per device before the first launch: the dynamic LDS limits of the bin kernel and of the three histogram kernels,
// each raised by the file that holds the kernel (raising one that a call never launches changes nothing).  Return a
// hipError_t.
int grow_lds_limits();            // grow.hip
int grow_lds_limits_weighted();   // grow_weighted.hip
int grow_lds_limits_sampled();    // grow_sampled.hip
inline int prepare_grow() {
  int e = grow_lds_limits();
  if (e == 0) e = grow_lds_limits_weighted();
  if (e == 0) e = grow_lds_limits_sampled();
  return e;
}
// The same for the pair path's histogram kernel (grow_pairs.hip), once per device before the first call that takes the
// pair path and not before: a call at default settings touches nothing of that file, its code object included.
int grow_lds_limits_pairs();
// Enqueues the binning.  bins must be sized by the plan.  Returns a hipError_t.
int launch_grow_bin(const GrowArgs& a, const GrowPlan& plan, void* stream);
// Enqueue one tree, round `round`: per level the histogram memsets, the histogram, split and partition kernels, then
// the leaf kernel (pred += leaf, pos = 0); the one level loop is grow_device.hpp's.  pos must be zero and pred the
// margin so far.  `plan` serves the partition and leaf kernels; `levels` the histogram kernel: plan_grow's for
// launch_grow_tree, plan_grow_weighted's for the other two, over the n_sel features of a sampled call (else `plan`
// itself).  Return a hipError_t.
int launch_grow_tree(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream);
int launch_grow_tree_weighted(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream);
int launch_grow_tree_sampled(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream);
// launch_grow_tree_weighted without the leaf kernel: the rows stay on their nodes after the last level's partition
int launch_grow_levels_weighted(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream);
// launch_grow_tree_sampled without the leaf kernel, likewise
int launch_grow_levels_sampled(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream);
// Enqueue grow_partition_kernel and grow_leaf_kernel alone, for the level loop as the other files instantiate it: they
// read node records and bins, never a histogram or a weight.  Return a hipError_t.
int launch_grow_partition(const GrowArgs& a, const GrowPlan& plan, uint32_t round, void* stream);
int launch_grow_leaf(const GrowArgs& a, const GrowPlan& plan, uint32_t round, void* stream);
// Enqueues grow_bag_kernel: the bit plane of the tree with a.row_key.  a.bag must not be nullptr.  Returns a hipError_t.
int launch_grow_bag(const GrowArgs& a, const GrowPlan& plan, void* stream);

// The metric kernels.  sums is [rounds + 1][2 sets: training, held-out][hi, lo] (grow_eval.hip); with weights
// (grow_weighted.hip) wsums is [2 sets] W, then [rounds + 1][2 sets][p2, p1, p0], and sums is not read.
struct GrowEvalArgs {
  const uint8_t* bins = nullptr;   // [num_feature][nrow] of the rows walked (the walk kernels only)
  float* pred = nullptr;           // [nrow] their running margin
  const float* labels = nullptr;   // [nrow]
  uint64_t nrow = 0;
  uint32_t num_feature = 0;
  const GrowNode* nodes = nullptr;       // [rounds][kGrowMaxNodes]
  const uint32_t* tree_nodes = nullptr;  // [rounds]
  unsigned long long* sums = nullptr;
  GrowLevelState* state = nullptr;
  int max_depth = 0;
  uint32_t label_flag = 0;         // what a residual out of range raises: kGrowFlagLabel or kGrowFlagEvalLabel
  const float* weights = nullptr;  // [nrow], or nullptr
  unsigned long long* wsums = nullptr;
  uint32_t weight_flag = 0;        // what a weight out of range raises: kGrowFlagWeight or kGrowFlagEvalWeight
};
constexpr uint32_t kGrowEvalTrain = 0, kGrowEvalHeldOut = 1;
inline size_t grow_sum_index(uint32_t t, uint32_t set) { return ((size_t)t * 2 + set) * 2; }
inline size_t grow_sum_count(size_t rounds) { return (rounds + 1) * 2 * 2; }
inline size_t grow_wide_index(uint32_t t, uint32_t set) { return 2 + ((size_t)t * 2 + set) * 3; }
inline size_t grow_wide_count(size_t rounds) { return 2 + (rounds + 1) * 2 * 3; }
// Enqueues grow_sse_kernel: sums[t][set] += the squares of pred - labels over the rows of `a`.  Returns a hipError_t.
int launch_grow_sse(const GrowEvalArgs& a, uint32_t blocks, uint32_t t, uint32_t set, void* stream);
// Enqueues grow_walk_sse_kernel: the rows of `a` walk tree `round` by their bins, pred += leaf, and
// sums[round + 1][set] += the squares.  Returns a hipError_t.
int launch_grow_walk_sse(const GrowEvalArgs& a, uint32_t blocks, uint32_t round, uint32_t set, void* stream);
// Enqueues grow_sse_weighted_kernel: wsums[t][set] += hq * e^2 over the rows of `a`; t == 0 also checks the weights
// and adds W of the set.  Returns a hipError_t.
int launch_grow_sse_weighted(const GrowEvalArgs& a, uint32_t blocks, uint32_t t, uint32_t set, void* stream);
// Enqueues grow_walk_sse_weighted_kernel: grow_walk_sse_kernel's walk, then wsums[round + 1][set] += hq * e^2.
int launch_grow_walk_sse_weighted(const GrowEvalArgs& a, uint32_t blocks, uint32_t round, uint32_t set, void* stream);

// ---- the Deep call (grow_deep.hip) ----

constexpr size_t kGrowEvalNodeBytes = 16;   // an EvalNode of grow_device.hpp: a node as the held-out walk reads it
// What the deep kernels take: the call's GrowArgs with `nodes` and `tree_nodes` at the call's first round, Ghist / Hhist
// the scratch of one batch and `best` the candidates of a whole level, and what the deep levels add.  With g.features
// (OHXBoosterBoostTreesDeepSampled) the histograms and `best` are compact over g.n_sel columns and g.bag, where it is
// not nullptr, is the bag of the tree at hand.
struct GrowDeepArgs {
  GrowArgs g;
  uint32_t* pos = nullptr;         // [nrow] the node a row stands on from level 8 on
  uint32_t node_stride = 0;        // node records of one round
  void* eval_nodes = nullptr;      // [node_stride] EvalNodes: the tree at hand as the held-out walk reads it
};
// One tree of a call with max_depth > 8, round `round`: levels 0 - 7 by launch_grow_levels_weighted (with g.features, by
// launch_grow_levels_sampled) on the tree's own records, then per deep level the batches (two memsets, the histogram
// kernel and split phase 0 each, of the kind), split phase 1, the partition, and one wait for the level word on h_state
// (pinned); then the leaf kernel.  The tree ends at the first level without an open node.  a.g.pos and a.pos must be
// zero and pred the margin so far.  Returns a hipError_t.
int launch_grow_tree_deep(const GrowDeepArgs& a, const GrowDeepPlan& plan, uint32_t round, GrowLevelState* h_state, void* stream);
// What differs between the Deep call's inline path and its pair path (grow_pairs.hip), as launches: `top` enqueues levels
// 0 - 7 without the leaf kernel on the tree's own records (round 0 of its own table and list) and returns a hipError_t;
// `hist` enqueues the histogram kernel of one batch of a deep level.  The level loop, its waits, the split phases of the
// deep levels (they read histograms alone) and the widen, partition and leaf kernels are launch_grow_tree_deep's own.
struct GrowDeepLaunches {
  std::function<int(const GrowArgs& top, const GrowPlan& lds, void* stream)> top;
  std::function<void(const GrowDeepArgs& d, uint32_t level, uint32_t round, uint32_t batch0, uint32_t nslots, uint32_t hist_blocks,
                     void* stream)>
      hist;
  // The histogram columns of the deep levels where they are not the tree's (0: they are): a column-sampled call's n_lvl.
  // The memsets, the waves of phase 0 and the plan's scratch are over them.
  uint32_t ncols = 0;
  // The split phases of a deep level, where they are not grow_deep.hip's own (empty: they are): phase 0 over `blocks`
  // blocks of four waves for the batch from batch0 on, and phase 1, one block.
  std::function<void(const GrowDeepArgs& d, uint32_t level, uint32_t round, uint32_t batch0, uint32_t blocks, void* stream)> split0;
  std::function<void(const GrowDeepArgs& d, uint32_t level, uint32_t round, void* stream)> split1;
};
// Enqueues grow_deep_stage_kernel alone: eval_nodes from the records of tree `round`.  Returns a hipError_t.
int launch_grow_deep_stage(const GrowDeepArgs& d, uint32_t blocks, uint32_t round, void* stream);
int launch_grow_tree_deep_with(const GrowDeepArgs& a, const GrowDeepPlan& plan, uint32_t round, GrowLevelState* h_state,
                               void* stream, const GrowDeepLaunches& launches);

// ---- the pair path (grow_pairs.hip; design in docs/26_objectives.md) ----

// What the pair kernels take beyond GrowArgs: the planes the pair kernel writes once a round and the histogram kernels
// read, the objective, and the list that stands for "every feature" where the call has no list of its own.
struct GrowPairArgs {
  long long* q = nullptr;            // [nrow] rint(g * w * 2^24)
  uint32_t* hq = nullptr;            // [nrow] rint(h * w * 2^24)
  const uint8_t* identity = nullptr; // [num_feature] 0 .. F - 1
  uint32_t objective = kGrowObjSquared;
  float slope = 1.0f;
};
// What a root with H == 0 raises at level 0 (the ROOT of the pair path's split kernels): nothing (the weighted call at
// squared error), kGrowFlagBag (the sampled call at squared error) or kGrowFlagHess (pseudo-Huber, bag or no bag).
constexpr int kGrowRootNone = 0, kGrowRootBag = 1, kGrowRootHess = 2;
// The split launches of the pair path where they are not its own (grow_reg.hip gives its regularised ones): levels 0 - 7
// over the columns `list[0 .. ncols)` - phase 0 over `blocks` blocks of four waves, phase 1 one block with the call's
// `root` - and the deep levels' as GrowDeepLaunches takes them.  Everything else of a tree is launched as ever.
struct GrowPairSplits {
  std::function<void(const GrowArgs& a, const uint8_t* list, uint32_t ncols, uint32_t blocks, uint32_t level, uint32_t round, void* stream)> split0;
  std::function<void(const GrowArgs& a, const uint8_t* list, uint32_t ncols, int root, uint32_t level, uint32_t round, void* stream)> split1;
  std::function<void(const GrowDeepArgs& d, uint32_t level, uint32_t round, uint32_t batch0, uint32_t blocks, void* stream)> deep_split0;
  std::function<void(const GrowDeepArgs& d, uint32_t level, uint32_t round, void* stream)> deep_split1;
  // Column sampling by level (grow_colsample.hip): with levels.lists the histogram kernels of level d of the call's round
  // r add the columns levels.list(r, d), levels.n_lvl of them, in place of the tree's list, and so do the memsets and the
  // split launches; the call's plan is over n_lvl columns.  `list` and `ncols` of split0 / split1 are then the level's, and
  // level_split0 / level_split1 stand in their place: they take the call's round too, which `round` is not where the
  // tree is round 0 of its own table (the Deep call's levels 0 - 7).
  GrowColsampleArgs levels;
  std::function<void(const GrowArgs& a, uint32_t tree, uint32_t blocks, uint32_t level, uint32_t round, void* stream)> level_split0;
  std::function<void(const GrowArgs& a, uint32_t tree, int root, uint32_t level, uint32_t round, void* stream)> level_split1;
};
// launch_grow_tree_weighted (a.features == nullptr) or launch_grow_tree_sampled (a.features != nullptr) on pairs: the
// pair kernel over every row, then the levels with the histogram kernel that reads the planes, then the leaf kernel.
// With kGrowObjPseudoHuber a root without hessian raises kGrowFlagHess.  `splits`: nullptr, or the split launches to
// use in place of this file's.  Returns a hipError_t.
int launch_grow_tree_pairs(const GrowArgs& a, const GrowPairArgs& p, const GrowPlan& plan, const GrowPlan& levels, uint32_t round,
                           void* stream, const GrowPairSplits* splits = nullptr);
// The levels of launch_grow_tree_pairs alone, over planes that hold the round's pairs already: no pair kernel before them
// and no leaf kernel after, so the rows stay on their leaves (grow_quantile.hip, which makes the pairs and sets the leaves).
int launch_grow_levels_pairs(const GrowArgs& a, const GrowPairArgs& p, const GrowPlan& plan, const GrowPlan& levels, uint32_t round,
                             void* stream);
// launch_grow_tree_deep on pairs, with or without a bag and a list.  Returns a hipError_t.
int launch_grow_tree_deep_pairs(const GrowDeepArgs& a, const GrowPairArgs& p, const GrowDeepPlan& plan, uint32_t round,
                                GrowLevelState* h_state, void* stream, const GrowPairSplits* splits = nullptr);

// ---- reg_alpha, max_delta_step and the metrics on the GPU (grow_reg.hip; design in docs/27_regularisation_and_metrics.md) ----

// The regularised split launches of a call: grow_split_reg_kernel for levels 0 - 7 and grow_deep_split_reg_kernel below.
GrowPairSplits grow_reg_splits(const GrowRegHess& hess);
// launch_grow_sse_weighted, launch_grow_walk_sse_weighted and launch_grow_walk_sse_deep with the row's term of `metric`
// (kGrowMetricMae or kGrowMetricPseudoHuber; slope is delta) in place of the square: the same sums, flags and layout.
int launch_grow_sse_metric(const GrowEvalArgs& a, uint32_t metric, float slope, uint32_t blocks, uint32_t t, uint32_t set, void* stream);
int launch_grow_walk_sse_metric(const GrowEvalArgs& a, uint32_t metric, float slope, uint32_t blocks, uint32_t round, uint32_t set,
                                void* stream);
int launch_grow_walk_sse_deep_metric(const GrowEvalArgs& a, const GrowDeepArgs& d, uint32_t metric, float slope, uint32_t blocks,
                                     uint32_t round, uint32_t set, void* stream);
// ---- monotone constraints on the GPU (grow_mono.hip; design in docs/28_monotone_constraints.md) ----

// The constrained split launches of a call: grow_split_mono_kernel for levels 0 - 7 and grow_deep_split_mono_kernel below.
// m.bounds holds two doubles a node of the call's node stride, m.constraints num_feature entries; both on the device.
GrowPairSplits grow_mono_splits(const GrowMonoArgs& m);
// ---- column sampling by level and by node on the GPU (grow_colsample.hip; design in docs/29_colsample_level_node.md) ----

// The split launches of a column-sampled call under each hessian policy of the pair path: grow_split_colsample_kernel
// for levels 0 - 7 and grow_deep_split_colsample_kernel below, over the level's list, with a (node, column) outside the
// node's features left an invalid candidate.  c.lists is on the device.  Empty launches where c is unsound.
GrowPairSplits grow_colsample_splits(const GrowColsampleArgs& c, const GrowFixedHess& hess);
GrowPairSplits grow_colsample_splits(const GrowColsampleArgs& c, const GrowRegHess& hess);
GrowPairSplits grow_colsample_splits(const GrowColsampleArgs& c, const GrowMonoArgs& m);
// ---- interaction constraints on the GPU (grow_interact.hip; design in docs/35_interaction_constraints.md) ----

// The split launches of a call under interaction constraints, under each hessian policy of the pair path:
// grow_split_interact_kernel for levels 0 - 7 and grow_deep_split_interact_kernel below, over the tree's list, with a
// (node, column) outside the node's allowed set left an invalid candidate.  x.groups (x.ngroups x 2 words) and x.sets
// (four words a node of the call's node stride) are on the device.  Empty launches where x is unsound.
GrowPairSplits grow_interact_splits(const GrowInteractArgs<GrowFixedHess>& x);
GrowPairSplits grow_interact_splits(const GrowInteractArgs<GrowRegHess>& x);
GrowPairSplits grow_interact_splits(const GrowInteractArgs<GrowMonoArgs>& x);
// Enqueues grow_deep_stage_kernel and grow_deep_walk_sse_kernel: eval_nodes from the records of tree `round`, then
// launch_grow_walk_sse_weighted's walk and sums over the rows of `a`, its nodes read from HBM.  Returns a hipError_t.
int launch_grow_walk_sse_deep(const GrowEvalArgs& a, const GrowDeepArgs& d, uint32_t blocks, uint32_t round, uint32_t set,
                              void* stream);
#endif  // __HIPCC__

}  // namespace ohx
