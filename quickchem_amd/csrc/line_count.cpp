// Distinct cache lines per deep gather of the super-node walk, priced on the host (docs/04_tree_walk_cost.md §4.13).
// A gather costs the texture path by the tag look-ups of its quads and by the lines that miss the L1; both are decided
// by where emit_super put the groups (flatten.hpp kSuperPack*) and by which rows share a wave, and neither needs a GPU
// to be counted.  The rows go through the trees with the host walk of the layout tests (super_walk.hpp) and to the
// lanes as the ring kernels send them (walk_device.hpp tile_row).
#include <algorithm>
#include <cmath>
#include <vector>

#include "super_walk.hpp"

namespace ohx {

namespace {

// lane -> gridcell of its brick, in grid order: what tile_row (walk_device.hpp) does with a lane
inline uint32_t lane_cell(const LineCountShape& sh, uint32_t l) {
  if (sh.li + sh.lj + sh.lk != 6) return l;
  uint32_t di, dj, dk;
  if (sh.k_fastest) {
    dk = l & ((1u << sh.lk) - 1u);
    di = (l >> sh.lk) & ((1u << sh.li) - 1u);
    dj = l >> (sh.lk + sh.li);
  } else {
    di = l & ((1u << sh.li) - 1u);
    dj = (l >> sh.li) & ((1u << sh.lj) - 1u);
    dk = l >> (sh.li + sh.lj);
  }
  return di + (dj << sh.li) + (dk << (sh.li + sh.lj));
}

inline uint32_t distinct(uint32_t* v, uint32_t n) {
  std::sort(v, v + n);
  return (uint32_t)(std::unique(v, v + n) - v);
}

}  // namespace

void count_super_lines(const SuperForest& sf, uint32_t num_feature, const float* rows, uint64_t ntile, uint32_t ncol,
                       float missing, const LineCountShape& shape, uint32_t first_step, LineCountStep* steps) {
  constexpr uint32_t kLanes = 64, kBlockTiles = 16;
  const uint64_t nblock = (ntile + kBlockTiles - 1) / kBlockTiles;
  std::vector<LineCountStep> total(kLineCountMaxSteps);
  std::string failed;   // what a walk threw: no exception may leave a parallel region
#pragma omp parallel
  {
    std::vector<LineCountStep> mine(kLineCountMaxSteps);
    std::vector<float> x((size_t)kBlockTiles * kLanes * 32);
    // record read per [step][tile of the block][lane], as an index into the whole array (the device copy is 128-byte
    // aligned: record r lies in block r / 4 and line r / 8)
    std::vector<uint32_t> where((size_t)kLineCountMaxSteps * kBlockTiles * kLanes);
    std::vector<uint32_t> trace(kLineCountMaxSteps), scratch((size_t)kBlockTiles * kLanes);
#pragma omp for schedule(dynamic, 1)
    for (int64_t b = 0; b < (int64_t)nblock; ++b) try {
      const uint64_t tile0 = (uint64_t)b * kBlockTiles;
      const uint32_t tiles = (uint32_t)std::min<uint64_t>(kBlockTiles, ntile - tile0);
      for (uint32_t w = 0; w < tiles; ++w)
        for (uint32_t l = 0; l < kLanes; ++l)
          super_walk_row(rows + ((tile0 + w) * kLanes + lane_cell(shape, l)) * ncol, ncol, num_feature, missing,
                         &x[((size_t)w * kLanes + l) * 32]);
      for (const SuperTreeHead& h : sf.heads) {
        const uint32_t nsteps = std::min(h.steps, kLineCountMaxSteps);
        if (nsteps <= first_step) continue;
        for (uint32_t w = 0; w < tiles; ++w)
          for (uint32_t l = 0; l < kLanes; ++l) {
            super_walk_tree(sf, h, &x[((size_t)w * kLanes + l) * 32], nsteps, trace.data());
            for (uint32_t s = first_step; s < nsteps; ++s)
              where[((size_t)s * kBlockTiles + w) * kLanes + l] = h.base + trace[s];
          }
        for (uint32_t s = first_step; s < nsteps; ++s) {
          LineCountStep& st = mine[s];
          const uint32_t* at = &where[(size_t)s * kBlockTiles * kLanes];
          for (uint32_t w = 0; w < tiles; ++w) {
            const uint32_t* lane = at + (size_t)w * kLanes;
            st.gathers += 1;
            std::copy(lane, lane + kLanes, scratch.begin());
            st.records += distinct(scratch.data(), kLanes);
            for (uint32_t q = 0; q < kLanes; q += 4) {
              uint32_t blk[4] = {lane[q] >> 2, lane[q + 1] >> 2, lane[q + 2] >> 2, lane[q + 3] >> 2};
              st.lookups += distinct(blk, 4);
            }
            for (uint32_t l = 0; l < kLanes; ++l) scratch[l] = lane[l] >> 3;
            st.lines += distinct(scratch.data(), kLanes);
          }
          if (tiles == kBlockTiles) {
            for (uint32_t i = 0; i < kBlockTiles * kLanes; ++i) scratch[i] = at[i] >> 3;
            st.block_gathers += 1;
            st.block_lines += distinct(scratch.data(), kBlockTiles * kLanes);
          }
        }
      }
    } catch (const std::exception& e) {
#pragma omp critical
      failed = e.what();
    }
#pragma omp critical
    for (uint32_t s = 0; s < kLineCountMaxSteps; ++s) {
      total[s].gathers += mine[s].gathers;
      total[s].records += mine[s].records;
      total[s].lookups += mine[s].lookups;
      total[s].lines += mine[s].lines;
      total[s].block_gathers += mine[s].block_gathers;
      total[s].block_lines += mine[s].block_lines;
    }
  }
  if (!failed.empty()) throw OhxError(failed);
  for (uint32_t s = 0; s < kLineCountMaxSteps; ++s) steps[s] = total[s];
}

}  // namespace ohx
