// libohx_synth.so: the two host decisions of the predict path that only choose how rows share a wave (kernels.hpp), for
// the CPU test-suite - the order of the rows from the clustering pass's nine words, and the level size adopted from the
// level search's verdict words.  Test support: the product calls the same inline functions from capi.cpp.
#include <cstdint>

#include "kernels.hpp"

#pragma GCC visibility push(default)
extern "C" {

// out[0] = order, out[1] = observed, out[2] = by chance; returns 1 where rows of that order are clustered, else 0
int ohx_cluster_order(const uint32_t* agree9, uint64_t nrow, double* out) {
  out[0] = ohx::cluster_order(agree9, nrow, &out[1], &out[2]);
  return out[0] < ohx::kClusterOrderBelow ? 1 : 0;
}

// verdict: 4 x (kmax - 1) words as launch_detect_period leaves them; the period adopted, 0 for none
uint64_t ohx_pick_level_period(const uint32_t* verdict, uint32_t kmax, uint64_t nrow) {
  return ohx::pick_level_period(verdict, kmax, nrow);
}

}  // extern "C"
#pragma GCC visibility pop
