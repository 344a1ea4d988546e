// Quantile cuts from rows in HBM (include/ohxgb.h OHXDMatrixQuantileCuts; design in docs/19_device_cuts.md): the cuts
// OHXQuantileCuts makes, found without a sort.  A cut is either a distinct value of its column or an order statistic
// s[floor(j * n / max_bins)]; both are found exactly by an integer radix select that looks for all ranks at once.  A
// float becomes an order-preserving 32-bit key; three passes over the sampled rows count 12, 10 and 10 key bits into
// integer histograms; between two passes a column keeps at most 255 selected key prefixes, and per target rank the
// slot of its prefix and its residual rank within it.  While a column has shown no more than max_bins distinct
// prefixes ("alive") every prefix is selected, so that after the last pass the selection is the column's distinct
// values; otherwise only the targets' prefixes are.  Integer adds only: the result depends on neither the order of
// the rows nor the launch shape.
//
// What host and device share is in this header: the key, the keep rule, the slot search, locating a rank in a row of
// digit counts, the alive rule and the launch plan.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define OHX_CUTS_HD __host__ __device__
#else
#define OHX_CUTS_HD
#endif

namespace ohx {

constexpr uint32_t kCutsMaxBins = 255;         // max_bins at most: targets and selected prefixes per column
constexpr uint32_t kCutsSlots = 256;           // the arrays of a column record
constexpr uint32_t kCutsSelStride = 255;       // a column's staged prefixes in LDS
constexpr uint32_t kCutsBits1 = 12, kCutsBits2 = 10, kCutsBits3 = 10;   // the device's digits
constexpr uint32_t kCutsDigits1 = 1u << kCutsBits1;   // 4096
constexpr uint32_t kCutsDigits = 1u << kCutsBits2;    // 1024, passes 2 and 3
constexpr uint64_t kCutsMaxRows = 1ull << 31;

// The order-preserving key of a float's bits: -0.0f counts as +0.0f, negative floats are flipped whole, the others get
// their sign bit set.  Integer operations only: a denormal is never flushed.
OHX_CUTS_HD inline uint32_t cuts_key(uint32_t u) {
  if (u == 0x80000000u) u = 0u;
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
OHX_CUTS_HD inline uint32_t cuts_unkey(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

OHX_CUTS_HD inline uint32_t cuts_float_bits(float v) { return __builtin_bit_cast(uint32_t, v); }

// Step (1) of the header: a value counts when it is not NaN, not == missing (a float compare) and finite.
OHX_CUTS_HD inline bool cuts_keep(float v, float missing, bool missing_is_nan) {
  if (v != v || (!missing_is_nan && v == missing)) return false;
  return (cuts_float_bits(v) & 0x7FFFFFFFu) != 0x7F800000u;
}

// The slot of `prefix` among the n ascending selected prefixes, or n where it is not selected.
OHX_CUTS_HD inline uint32_t cuts_find_slot(const uint32_t* sel, uint32_t n, uint32_t prefix) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sel[mid] < prefix) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && sel[lo] == prefix) ? lo : n;
}

// The digit that holds rank *rank (0-based) among the values counted in row[0 .. digits); the counts of the digits
// below it are taken off *rank.  Returns `digits` when the row holds no more than *rank values (never, from sound
// counts).
OHX_CUTS_HD inline uint32_t cuts_locate(const uint32_t* row, uint32_t digits, uint32_t* rank) {
  uint32_t r = *rank;
  for (uint32_t d = 0; d < digits; ++d) {
    const uint32_t c = row[d];
    if (r < c) {
      *rank = r;
      return d;
    }
    r -= c;
  }
  *rank = r;
  return digits;
}

// The rank of target j among n kept values: target 0 is the minimum, target j the candidate of step (4).
OHX_CUTS_HD inline uint32_t cuts_target_rank(uint32_t j, uint32_t n, uint32_t max_bins) {
  return (uint32_t)((uint64_t)j * n / max_bins);
}

// A column stays alive while the prefixes seen so far - the nonzero counters of a pass that selected all of them - are
// no more than max_bins.
OHX_CUTS_HD inline bool cuts_alive_after(bool alive, uint64_t nonzero, uint32_t max_bins) {
  return alive && nonzero <= max_bins;
}

// A column between two passes, and what the host reads back after the last.
struct CutsCol {
  uint32_t n;                    // kept values (set after pass 1)
  uint32_t alive;
  uint32_t nsel;                 // selected prefixes, ascending in sel[]
  uint32_t error;                // a rank that its counters do not hold (never, from sound counters)
  uint32_t sel[kCutsSlots];
  uint32_t tslot[kCutsSlots];    // per target j < max_bins: the slot of its prefix
  uint32_t trank[kCutsSlots];    // and its rank among the values of that prefix
};

// ---- the host side (cuts.cpp) ----

// The between-pass step on the host: `table` holds [col.nsel (1 before the first pass)][digits] counters of the pass
// just done; col is advanced to the next pass (n is set when first is true).
void cuts_select_step(CutsCol& col, const uint32_t* table, uint32_t bits, uint32_t max_bins, bool first);
// Steps (2)-(4) of the header from a column's record after the last pass; the cut values are appended.
void cuts_assemble(const CutsCol& col, uint32_t max_bins, std::vector<float>& cuts);
// Writes cut_ptr (ncol + 1) always and cut_values where they fit `cap` from the columns' records; returns the number
// of cut values.
uint64_t cuts_write(const CutsCol* cols, uint64_t ncol, uint32_t max_bins, uint64_t* cut_ptr, float* cut_values, uint64_t cap);
// The whole select on the host, for rows 0, row_step, 2 * row_step, ... of the row-major data: the counting is a
// plain loop, the step between passes is cuts_select_step.  bits: the digits of the passes, summing to 32, each 1..16.
uint64_t cuts_select_host(const float* data, uint64_t nrow, uint64_t ncol, float missing, int max_bins, uint64_t row_step,
                          const uint32_t* bits, uint32_t npass, uint64_t* cut_ptr, float* cut_values, uint64_t cap);

// ---- the launch plan ----

constexpr uint32_t kCutsBlock = 1024;          // the counting kernels: sixteen waves, a sampled row per lane
constexpr uint32_t kCutsSelectBlock = 256;     // the select kernel: one block per column
constexpr uint32_t kCutsBlocksPerCu = 2;       // over all of gridDim.y
constexpr uint32_t kCutsLdsBytes = 160 * 1024; // a CU's LDS
constexpr uint32_t kCutsMaxGroup1 = kCutsLdsBytes / (kCutsDigits1 * 4);   // 10 columns' histograms in pass 1
constexpr uint32_t kCutsMaxGroup = 128;        // columns whose prefixes are staged together in passes 2 and 3

struct CutsPlan {
  uint64_t sampled = 0;        // rows 0, row_step, ... below nrow
  uint32_t blocks1 = 0;        // pass 1: gridDim.x, blocks over the sampled rows
  uint32_t col_group1 = 0, col_groups1 = 0;   // pass 1: columns per block, gridDim.y
  uint32_t lds1_bytes = 0;     // col_group1 x 4096 x 4
  uint32_t blocks = 0;         // passes 2 and 3: gridDim.x
  uint32_t col_group = 0, col_groups = 0;     // passes 2 and 3
  uint32_t lds_bytes = 0;      // the staged prefixes: col_group x 255 x 4
  uint64_t table1_bytes = 0;   // ncol x 4096 x 4
  uint64_t table_bytes = 0;    // ncol x 255 x 1024 x 4
};
CutsPlan plan_cuts(uint64_t nrow, uint64_t row_step, uint64_t ncol, int num_cus);

#ifdef __HIPCC__
struct CutsArgs {
  const float* rows = nullptr;   // [nrow][ncol]
  uint64_t sampled = 0, row_step = 1;
  uint32_t ncol = 0;
  float missing = 0.0f;
  uint32_t max_bins = 0;
  uint32_t* table1 = nullptr;    // [ncol][4096]
  uint32_t* table = nullptr;     // [ncol][255][1024]
  CutsCol* cols = nullptr;       // [ncol]
};
// Once per device before the first launch: the dynamic LDS limits.  Returns a hipError_t.
int prepare_cuts();
// Enqueues the whole select: the memsets, three counting kernels and the select kernel after each.  The records in
// a.cols are complete when the stream has run.  Returns a hipError_t.
int launch_cuts(const CutsArgs& a, const CutsPlan& plan, void* stream);
#endif  // __HIPCC__

}  // namespace ohx
