// Selected gridcells (cells.hip; include/ohxgb.h OHXSelectCells, OHXGatherCells, OHXScatterCells): choose cells of an
// (im,jm,km) block on the device, gather their rows from the fields into a row matrix, scatter per-cell results back.
// A cell index is c = (i-1) + im*((j-1) + jm*(k-1)), int64.  No booster is involved.
#pragma once

#include <cstdint>

namespace ohx {

// bits the kernels OR into a caller's status word
constexpr uint32_t kCellsOutOfRange = 1u;       // a cell index outside [0, im*jm*km)
constexpr uint32_t kCellsNotAscending = 2u;     // the scatter's cells are not strictly ascending
constexpr uint32_t kCellsOverCap = 4u;          // the selection did not fit cap

constexpr uint32_t kCellsWave = 64;
constexpr uint32_t kCellsBlock = 256;           // threads of a selection / scatter block
constexpr uint32_t kCellsMaxBlocks = 4096;      // most blocks of such a launch: the size of the per-block table
constexpr uint32_t kCellsMaxFields = 32;

// How an ordered pass over `n` items is cut: `blocks` blocks of kCellsBlock threads, block b owning the contiguous
// items [b * chunk, min(n, (b + 1) * chunk)), chunk a multiple of kCellsBlock.  The selection's box cells and the
// scatter's list entries are both cut this way; n == 0 gives no block.
struct CellsPassPlan {
  uint32_t blocks = 0;
  uint64_t chunk = 0;
};
inline CellsPassPlan plan_cells_pass(uint64_t n) {
  CellsPassPlan p;
  if (n == 0) return p;
  const uint64_t per = (n + kCellsMaxBlocks - 1) / kCellsMaxBlocks;
  p.chunk = (per + kCellsBlock - 1) / kCellsBlock * kCellsBlock;
  p.blocks = (uint32_t)((n + p.chunk - 1) / p.chunk);
  return p;
}

// Floats between the rows of two neighbouring lanes in the gather's LDS tile: nfield made odd, so that the 32 lanes
// ds_write_b32 serves together (banks = dword address mod 32) land on 32 different banks when each writes its own
// row's column f.
inline uint32_t cells_gather_lds_stride(uint32_t nfield) { return nfield | 1u; }

struct SelectCellsArgs {
  int64_t im = 0, jm = 0;
  int64_t i0 = 0, j0 = 0, k0 = 0;     // the box's first cell, 0-based
  int64_t wi = 0, wj = 0, wk = 0;     // its extents
  const float* a = nullptr;           // device; null: every cell of the box
  const float* b = nullptr;           // device; null: b0
  int32_t a_is2d = 0, b_is2d = 0;
  float b0 = 0.0f;
  int64_t* cells = nullptr;           // device, cap entries
  int64_t cap = 0;
  int64_t* count = nullptr;           // device
  uint32_t* status = nullptr;         // device, may be null
};
// `table` holds kCellsMaxBlocks uint64 for the life of the launches (device).  Enqueues on `stream` (a hipStream_t):
// the count pass, then the pass that writes.  An empty box only writes the count.  Returns a hipError_t.
int launch_select_cells(const SelectCellsArgs& a, uint64_t* table, void* stream);

struct GatherCellsArgs {
  const float* field[kCellsMaxFields];   // device; field f is (im,jm) when bit f of is2d_mask is set
  uint32_t is2d_mask = 0;
  uint32_t pl_feature = 0xFFFFFFFFu;     // divided by 100 (0xFFFFFFFF: none)
  uint32_t nfield = 0;
  int64_t plane = 0;                     // im * jm
  int64_t ncells_total = 0;              // im * jm * km
};
int launch_gather_cells(const GatherCellsArgs& g, const int64_t* cells, int64_t ncell, float* rows, uint32_t* status,
                        void* stream);

// out3d[cells[n]] = values[n * stride + col] for every n whose cell is in range and above every earlier entry.
// `table` as for the selection.
int launch_scatter_cells(const float* values, int64_t stride, int64_t col, const int64_t* cells, int64_t ncell,
                         float* out3d, int64_t ncells_total, uint32_t* status, uint64_t* table, void* stream);

}  // namespace ohx
