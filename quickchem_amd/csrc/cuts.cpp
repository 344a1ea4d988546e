// Host side of the device quantile cuts (cuts.hpp): the step between two passes as the select kernel takes it, the
// final assembly of a column's cuts from its record, a host driver of the whole select whose counting is a plain loop,
// and the launch plan.  No device code: libohx_synth.so links it too, for the tests that need no GPU.
#include "cuts.hpp"

#include <algorithm>
#include <string>

#include "forest.hpp"

namespace ohx {

void cuts_select_step(CutsCol& col, const uint32_t* table, uint32_t bits, uint32_t max_bins, bool first) {
  const uint32_t D = 1u << bits;
  if (first) {
    uint64_t n = 0;
    for (uint32_t d = 0; d < D; ++d) n += table[d];
    col.n = (uint32_t)n;
    col.alive = 1;
    col.nsel = 1;
    col.error = 0;
    col.sel[0] = 0;
    for (uint32_t j = 0; j < max_bins; ++j) {
      col.tslot[j] = 0;
      col.trank[j] = cuts_target_rank(j, col.n, max_bins);
    }
  }
  const uint32_t nsel = col.nsel;
  // every target steps to the digit that holds its rank
  uint32_t prefix[kCutsSlots];
  if (col.n != 0) {
    for (uint32_t j = 0; j < max_bins; ++j) {
      const uint32_t slot = col.tslot[j];
      uint32_t rank = col.trank[j];
      uint32_t d = slot < nsel ? cuts_locate(table + (size_t)slot * D, D, &rank) : D;
      if (d == D) {
        col.error = 1;
        d = D - 1;
      }
      prefix[j] = (col.sel[slot < nsel ? slot : 0] << bits) | d;
      col.trank[j] = rank;
    }
  }
  uint64_t nonzero = 0;
  if (col.alive)
    for (size_t i = 0; i < (size_t)nsel * D; ++i) nonzero += table[i] != 0u ? 1u : 0u;
  const bool alive = cuts_alive_after(col.alive != 0, nonzero, max_bins);
  // the next selection: every prefix seen while alive, else the targets' own
  uint32_t next[kCutsSlots];
  uint32_t k = 0;
  if (alive) {
    for (uint32_t s = 0; s < nsel; ++s)
      for (uint32_t d = 0; d < D; ++d)
        if (table[(size_t)s * D + d] != 0u) next[k++] = (col.sel[s] << bits) | d;
  } else if (col.n != 0) {
    for (uint32_t j = 0; j < max_bins; ++j)
      if (j == 0 || prefix[j] != prefix[j - 1]) next[k++] = prefix[j];
  }
  for (uint32_t i = 0; i < k; ++i) col.sel[i] = next[i];
  col.nsel = k;
  col.alive = alive ? 1u : 0u;
  if (col.n != 0) {
    for (uint32_t j = 0; j < max_bins; ++j) {
      col.tslot[j] = cuts_find_slot(col.sel, k, prefix[j]);
      if (col.tslot[j] >= k) col.error = 1;
    }
  }
}

namespace {
float key_value(uint32_t key) {
  const uint32_t u = cuts_unkey(key);
  float v;
  memcpy(&v, &u, sizeof v);
  return v;
}
}  // namespace

void cuts_assemble(const CutsCol& col, uint32_t max_bins, std::vector<float>& cuts) {
  if (col.error != 0) throw OhxError("quantile cuts: a column's counters do not hold one of its ranks");
  if (col.n == 0) return;
  if (col.alive) {
    // m = nsel <= max_bins distinct values: none for m <= 1, else u_1 .. u_{m-1}
    for (uint32_t i = 1; i < col.nsel; ++i) cuts.push_back(key_value(col.sel[i]));
    return;
  }
  const uint32_t k0 = col.sel[col.tslot[0]];
  uint32_t last = k0;
  for (uint32_t j = 1; j < max_bins; ++j) {
    const uint32_t k = col.sel[col.tslot[j]];
    if (k == k0 || k == last) continue;
    cuts.push_back(key_value(k));
    last = k;
  }
}

uint64_t cuts_write(const CutsCol* cols, uint64_t ncol, uint32_t max_bins, uint64_t* cut_ptr, float* cut_values, uint64_t cap) {
  uint64_t total = 0;
  std::vector<float> cuts;
  cut_ptr[0] = 0;
  for (uint64_t c = 0; c < ncol; ++c) {
    cuts.clear();
    cuts_assemble(cols[c], max_bins, cuts);
    for (size_t i = 0; i < cuts.size(); ++i)
      if (total + i < cap) cut_values[total + i] = cuts[i];
    total += cuts.size();
    cut_ptr[c + 1] = total;
  }
  return total;
}

uint64_t cuts_select_host(const float* data, uint64_t nrow, uint64_t ncol, float missing, int max_bins, uint64_t row_step,
                          const uint32_t* bits, uint32_t npass, uint64_t* cut_ptr, float* cut_values, uint64_t cap) {
  uint32_t sum = 0;
  for (uint32_t p = 0; p < npass; ++p) {
    if (bits[p] < 1 || bits[p] > 16) throw OhxError("cuts_select_host: a pass takes 1 to 16 bits");
    sum += bits[p];
  }
  if (npass == 0 || sum != 32) throw OhxError("cuts_select_host: the passes' bits must sum to 32");
  if (max_bins < 2 || max_bins > (int)kCutsMaxBins) throw OhxError("cuts_select_host: max_bins must be in 2..255");
  if (row_step < 1) throw OhxError("cuts_select_host: row_step must be >= 1");
  const bool missing_is_nan = missing != missing;
  std::vector<CutsCol> cols(ncol);
  std::vector<uint32_t> table;
  for (uint64_t c = 0; c < ncol; ++c) {
    CutsCol& col = cols[c];
    memset(&col, 0, sizeof col);
    col.nsel = 1;   // the single empty prefix of the first pass
    uint32_t done = 0;
    for (uint32_t p = 0; p < npass; ++p) {
      const uint32_t b = bits[p], D = 1u << b, shift = 32 - done - b;
      table.assign((size_t)std::max<uint32_t>(col.nsel, 1) * D, 0u);
      for (uint64_t r = 0; r < nrow; r += row_step) {
        const float v = data[r * ncol + c];
        if (!cuts_keep(v, missing, missing_is_nan)) continue;
        const uint32_t key = cuts_key(cuts_float_bits(v));
        const uint32_t slot = p == 0 ? 0u : cuts_find_slot(col.sel, col.nsel, key >> (32 - done));
        if (slot >= col.nsel) continue;
        ++table[(size_t)slot * D + ((key >> shift) & (D - 1))];
      }
      cuts_select_step(col, table.data(), b, (uint32_t)max_bins, p == 0);
      done += b;
    }
  }
  return cuts_write(cols.data(), ncol, (uint32_t)max_bins, cut_ptr, cut_values, cap);
}

CutsPlan plan_cuts(uint64_t nrow, uint64_t row_step, uint64_t ncol, int num_cus) {
  CutsPlan p;
  const uint64_t cus = num_cus > 0 ? (uint64_t)num_cus : 1;
  const uint64_t step = std::max<uint64_t>(row_step, 1);
  p.sampled = (nrow + step - 1) / step;
  const uint32_t C = (uint32_t)std::max<uint64_t>(ncol, 1);
  const uint64_t want = (p.sampled + kCutsBlock - 1) / kCutsBlock;
  // the same number of groups, evenly filled, as plan_grow fills its feature groups
  p.col_groups1 = (C + kCutsMaxGroup1 - 1) / kCutsMaxGroup1;
  p.col_group1 = (C + p.col_groups1 - 1) / p.col_groups1;
  p.lds1_bytes = p.col_group1 * kCutsDigits1 * (uint32_t)sizeof(uint32_t);
  p.blocks1 = (uint32_t)std::max<uint64_t>(1, std::min(want, std::max<uint64_t>(1, cus * kCutsBlocksPerCu / p.col_groups1)));
  p.col_groups = (C + kCutsMaxGroup - 1) / kCutsMaxGroup;
  p.col_group = (C + p.col_groups - 1) / p.col_groups;
  p.lds_bytes = p.col_group * kCutsSelStride * (uint32_t)sizeof(uint32_t);
  p.blocks = (uint32_t)std::max<uint64_t>(1, std::min(want, std::max<uint64_t>(1, cus * kCutsBlocksPerCu / p.col_groups)));
  p.table1_bytes = (uint64_t)C * kCutsDigits1 * sizeof(uint32_t);
  p.table_bytes = (uint64_t)C * kCutsMaxBins * kCutsDigits * sizeof(uint32_t);
  return p;
}

}  // namespace ohx
