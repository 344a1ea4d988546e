// The host walk of the super-node layout (flatten.hpp): emit_super's arrays walked the way the kernels do - the root
// from the head record (phase 1), a fixed number of steps per tree, no finished state, the leaf taken whenever the
// child's code is 31, fillers after it.  Scalar, test support and host analysis only (synth_host.cpp ohx_super_walk_cpu,
// line_count.cpp); not a prediction path.
#pragma once
#include <cstring>
#include <string>

#include "flatten.hpp"

namespace ohx {

// One row through one tree.  x: the row's 32 feature values, missing = NaN.  nsteps: steps to take (a tree's own
// `steps` or more: a walk past its leaf only meets fillers).  trace, if given: the record each step read, relative to
// the tree's base, nsteps entries.  Returns the leaf value; throws where the layout breaks a promise of flatten.hpp.
inline float super_walk_tree(const SuperForest& sf, const SuperTreeHead& h, const float* x, uint32_t nsteps,
                             uint32_t* trace) {
  auto left = [](float xv, float thr, bool dl) { return xv != xv ? dl : xv < thr; };
  uint32_t rel = 4u;
  if (h.root_meta & 0x100u) rel += left(x[h.root_meta & 31u], h.root_thr, (h.root_meta & 32u) != 0) ? 0u : 1u;
  uint32_t leaf_bits = 0, taken = 0;
  for (uint32_t step = 0; step < nsteps; ++step) {
    // as walk_super does: the records of the first three steps among the tree's first kSuperTopSlots (its one "top"
    // load), and as the ring kernels do: those of the first four among its first kSuperRingSlots
    if (step < 3 && rel >= kSuperTopSlots) throw OhxError("tree top outside the first records of its tree");
    if (step < 4 && rel >= kSuperRingSlots) throw OhxError("a record of the first four steps outside the tree's first 176");
    if ((size_t)h.base + rel >= sf.nodes.size()) throw OhxError("walk left the super-node array");
    if (trace) trace[step] = rel;
    const SuperNode& s = sf.nodes[h.base + rel];
    const uint32_t w = s.meta;
    const bool l0 = left(x[(w >> 8) & 31u], s.thr0, ((w >> 5) & 1u) != 0);
    const float thr1 = l0 ? s.thrL : s.thrR;
    const uint32_t f1 = (w >> (l0 ? 0u : 13u)) & 31u;
    if (f1 == 31u) {
      memcpy(&leaf_bits, &thr1, 4);
      ++taken;
    }
    const bool l1 = left(x[f1], thr1, ((w >> (l0 ? 6u : 7u)) & 1u) != 0);
    rel = ((w >> 18) << 2) + (l0 ? 0u : 2u) + (l1 ? 0u : 1u);
  }
  if (taken != 1) throw OhxError("a walk must meet exactly one leaf code, met " + std::to_string(taken));
  float leaf;
  memcpy(&leaf, &leaf_bits, 4);
  return leaf;
}

// a row as the kernels see it: 32 values, `missing` and absent columns NaN, the values past the booster's features 0
inline void super_walk_row(const float* row, uint32_t ncol, uint32_t num_feature, float missing, float* x) {
  const bool missing_is_nan = missing != missing;
  for (uint32_t c = 0; c < 32; ++c) {
    float v = c < ncol ? row[c] : (c < num_feature ? NAN : 0.0f);
    if (c < ncol && !missing_is_nan && v == missing) v = NAN;
    x[c] = v;
  }
}

// Distinct cache lines of the deep gathers, counted on the host (line_count.cpp).
struct LineCountShape {
  uint32_t li = 0, lj = 0, lk = 0;   // the brick a wave takes, as TileShape (kernels.hpp); all 0: 64 consecutive rows
  uint32_t k_fastest = 0;            // lane order inside the brick, as TileShape::k_fastest
};
struct LineCountStep {               // sums over the wave-gathers of one step (a wave, a tree, a step)
  double gathers = 0;                // wave-gathers counted
  double records = 0;                // distinct 16-byte records among the 64 lanes
  double lookups = 0;                // distinct 64-byte blocks per quad of four consecutive lanes, summed over the 16 quads
  double lines = 0;                  // distinct 128-byte lines among the 64 lanes
  double block_gathers = 0;          // blocks of 16 neighbouring tiles x trees counted
  double block_lines = 0;            // distinct 128-byte lines among the 16 x 64 lanes of such a block
};
constexpr uint32_t kLineCountMaxSteps = 32;
// rows: [ntile][64][ncol], a tile's 64 gridcells in grid order (i fastest, then j, then k inside the brick), tiles in
// launch order: 16 consecutive tiles are one block's.  Counts steps first_step .. of every tree (0-based; the ring
// kernels gather from step 4 on).  steps[kLineCountMaxSteps].
void count_super_lines(const SuperForest& sf, uint32_t num_feature, const float* rows, uint64_t ntile, uint32_t ncol,
                       float missing, const LineCountShape& shape, uint32_t first_step, LineCountStep* steps);

}  // namespace ohx
