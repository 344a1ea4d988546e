// Test support (libohx_synth.so): the host pieces of the device quantile cuts (cuts.hpp) without a GPU - the whole
// select with its counting done in a plain loop and the between-pass step of cuts.cpp, the key, and the launch plan.
// The product library runs the same functions of cuts.hpp and cuts.cpp behind OHXDMatrixQuantileCuts.
#include <string>

#include "cuts.hpp"
#include "forest.hpp"

namespace ohx {
void synth_set_error(const std::string& m);   // synth_host.cpp
}

using namespace ohx;

// bits: npass digits summing to 32.  cut_ptr: ncol + 1.  Returns -1 with *needed set when more than cap are needed.
extern "C" __attribute__((visibility("default"))) int ohx_cuts_select(const float* data, uint64_t nrow, uint64_t ncol,
                                                                     float missing, int max_bins, uint64_t row_step,
                                                                     const uint32_t* bits, uint32_t npass, uint64_t* cut_ptr,
                                                                     float* cut_values, uint64_t cap, uint64_t* needed) {
  try {
    *needed = cuts_select_host(data, nrow, ncol, missing, max_bins, row_step, bits, npass, cut_ptr, cut_values, cap);
    if (*needed > cap)
      throw OhxError("ohx_cuts_select: " + std::to_string(*needed) + " cut values are needed and cut_values holds " +
                     std::to_string(cap));
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}

// keys[i] = cuts_key(bits[i]) and back[i] = cuts_unkey(keys[i])
extern "C" __attribute__((visibility("default"))) int ohx_cuts_keys(const uint32_t* bits, uint64_t n, uint32_t* keys,
                                                                   uint32_t* back) {
  for (uint64_t i = 0; i < n; ++i) {
    keys[i] = cuts_key(bits[i]);
    back[i] = cuts_unkey(keys[i]);
  }
  return 0;
}

// info: [0] sampled rows, [1] blocks of pass 1, [2] columns a pass-1 block takes, [3] column groups of pass 1, [4] LDS
// bytes of pass 1, [5] blocks of passes 2 and 3, [6] columns such a block takes, [7] their column groups, [8] LDS bytes
// of the staged prefixes, [9] bytes of the pass-1 table, [10] bytes of the table of passes 2 and 3, [11] rows a block
// takes per trip
extern "C" __attribute__((visibility("default"))) int ohx_cuts_plan(uint64_t nrow, uint64_t row_step, uint64_t ncol,
                                                                   int num_cus, uint64_t info[12]) {
  try {
    if (row_step < 1) throw OhxError("ohx_cuts_plan: row_step must be >= 1");
    const CutsPlan p = plan_cuts(nrow, row_step, ncol, num_cus);
    const uint64_t v[12] = {p.sampled,   p.blocks1,    p.col_group1, p.col_groups1,  p.lds1_bytes,  p.blocks,
                            p.col_group, p.col_groups, p.lds_bytes,  p.table1_bytes, p.table_bytes, kCutsBlock};
    for (int i = 0; i < 12; ++i) info[i] = v[i];
    return 0;
  } catch (const std::exception& e) {
    synth_set_error(e.what());
    return -1;
  }
}
