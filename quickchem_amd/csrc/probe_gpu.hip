// lib/libohx_synth_gpu.so: entry points that run, on the caller's own device buffers, the three pieces of the predict
// path that only decide which rows share a wave - the clustering keys and their `agree` words (kernels.hip
// launch_cluster_keys), the sort of the (key, row) pairs (sort_pairs.hip) and the level search's verdict words
// (kernels.hip launch_detect_period).  TEST SUPPORT, not the product: whatever these compute the margins stay bit-exact,
// so only a test that sees the keys, the permutation and the verdicts themselves can find them wrong
// (tests/test_gpu_cluster.py).  Linked with the very objects the product links (kernels.o, sort_pairs.o);
// libohxgb.so exports none of this.  Every pointer is a device pointer of the caller's; every function returns 0, or
// -1 with the reason in ohx_synth_gpu_last_error.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "kernels.hpp"

namespace ohx {
void synth_gpu_set_error(const std::string& m);   // synth_gpu.hip
}

namespace {

int fail(const std::string& m) {
  ohx::synth_gpu_set_error(m);
  return -1;
}

int checked(const char* what, hipError_t e) {
  return e == hipSuccess ? 0 : fail(std::string(what) + ": " + hipGetErrorName(e));
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

// d_super: emit_super's records (16 bytes each, super_bytes in all), d_heads: its num_trees tree heads, as
// ohx_super_records_cpu hands them out.  d_agree9 must be zero before (ClusterArgs::agree).  num_cus sizes the grid:
// with 1 a wave takes many tiles in turn.
int ohx_probe_cluster_keys(const void* d_super, uint64_t super_bytes, const void* d_heads, uint32_t num_trees,
                           uint32_t num_feature, const float* d_rows, uint64_t nrow, uint32_t ncol, float missing,
                           uint32_t ntrees, uint32_t nsteps, uint32_t zorder, uint32_t* d_keys, uint32_t* d_vals,
                           uint32_t* d_agree9, int num_cus, void* stream) {
  if (super_bytes > 0xFFFFFFFFull || super_bytes % sizeof(ohx::SuperNode) != 0) return fail("ohx_probe_cluster_keys: bad super_bytes");
  if (num_cus < 1) return fail("ohx_probe_cluster_keys: num_cus < 1");
  if (nrow && (d_rows == nullptr || d_keys == nullptr || d_vals == nullptr || d_agree9 == nullptr || d_heads == nullptr))
    return fail("ohx_probe_cluster_keys: a NULL pointer");
  ohx::DeviceForest fr;
  fr.super = static_cast<const ohx::SuperNode*>(d_super);
  fr.super_heads = static_cast<const ohx::SuperTreeHead*>(d_heads);
  fr.super_bytes = (uint32_t)super_bytes;
  fr.num_trees = num_trees;
  fr.num_feature = num_feature;
  ohx::ClusterArgs c;
  c.rows = d_rows;
  c.nrow = nrow;
  c.ncol = ncol;
  c.missing = missing;
  c.ntrees = ntrees;
  c.nsteps = nsteps;
  c.zorder = zorder;
  c.keys = d_keys;
  c.vals = d_vals;
  c.agree = d_agree9;
  return checked("launch_cluster_keys", ohx::launch_cluster_keys(fr, c, num_cus, static_cast<hipStream_t>(stream)));
}

// The calls of capi.cpp cluster_rows: the size query with no scratch, then the sort.  The scratch is allocated and
// freed in here (the stream has run when this returns).  *which = 0 / 1: d_vals_a / d_vals_b holds the sorted values.
int ohx_probe_sort_pairs(uint32_t* d_keys_a, uint32_t* d_keys_b, uint32_t* d_vals_a, uint32_t* d_vals_b, uint64_t n,
                         uint32_t key_bits, void* stream, int* which, uint64_t* temp_bytes) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  size_t bytes = 0;
  if (checked("sort_pairs_u32 (size query)",
              ohx::sort_pairs_u32(nullptr, &bytes, d_keys_a, d_keys_b, d_vals_a, d_vals_b, n, key_bits, s, nullptr)) != 0)
    return -1;
  if (temp_bytes) *temp_bytes = bytes;
  void* temp = nullptr;
  if (bytes > 0 && checked("hipMalloc", hipMalloc(&temp, bytes)) != 0) return -1;
  uint32_t* sorted = nullptr;
  int rc = checked("sort_pairs_u32", ohx::sort_pairs_u32(temp, &bytes, d_keys_a, d_keys_b, d_vals_a, d_vals_b, n, key_bits, s, &sorted));
  if (rc == 0) rc = checked("hipStreamSynchronize", hipStreamSynchronize(s));
  if (temp) (void)hipFree(temp);
  if (rc != 0) return rc;
  if (sorted != d_vals_a && sorted != d_vals_b) return fail("ohx_probe_sort_pairs: the result is in neither buffer");
  if (which) *which = sorted == d_vals_a ? 0 : 1;
  return 0;
}

// cols: `ncols` (<= 4) column numbers; d_verdict: ncols x (kmax - 1) words, zero before (kernels.hpp)
int ohx_probe_detect_period(const float* d_data, uint64_t nrow, uint32_t ncol, const uint32_t* cols, uint32_t ncols,
                            uint32_t kmax, uint32_t* d_verdict, void* stream) {
  if (ncols > 4 || cols == nullptr) return fail("ohx_probe_detect_period: one to four columns");
  if (d_data == nullptr || d_verdict == nullptr || nrow == 0 || ncol == 0) return fail("ohx_probe_detect_period: no rows");
  ohx::PeriodColumns pc{{0u, 0u, 0u, 0u}};
  for (uint32_t c = 0; c < ncols; ++c) pc.col[c] = cols[c];
  return checked("launch_detect_period",
                 ohx::launch_detect_period(d_data, nrow, ncol, pc, ncols, kmax, d_verdict, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
#pragma GCC visibility pop
