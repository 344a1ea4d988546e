// gfx950 kernels of boosters with several output groups (multi-class, multi-target; docs/13_output_groups.md).
//
// The walks and the contributions kernels run unchanged over one group's tree range at a time (the device copy of such
// a booster is ordered group by group, flatten.hpp group_major); what is left is putting the groups' results where
// xgboost 1.6.0's layouts want them.  Definitions in groups.hip, host side in capi.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace ohx {

// What group_finish writes for a row r from its G margins planes[g * nrow + r] (option_mask of XGBoosterPredict)
enum GroupFinish : int {
  kGroupMargins = 0,   // out[r * G + g] = margin                     (option_mask 1; 0 for an identity objective)
  kGroupSoftprob = 1,  // out[r * G + g] = softmax of the row's margins (option_mask 0, multi:softprob)
  kGroupArgmax = 2,    // out[r] = index of the row's first maximal margin, as float (option_mask 0, multi:softmax)
};

// Softmax as xgboost 1.6.0's common::Softmax (src/common/math.h) restates it, per row, groups in order 0 .. G-1:
//   wmax = max over g of the float margins (fmaxf, starting from group 0)
//   e_g  = expf(margin_g - wmax)                    float
//   wsum = sum of e_g in group order                 accumulated in DOUBLE, from 0.0
//   out_g = e_g / (float)wsum                        float division
// Argmax as 1.6.0's common::FindMaxIndex (std::max_element): the first g whose margin no later one exceeds.
hipError_t launch_group_finish(const float* planes, uint64_t nrow, uint32_t G, int mode, float* out, hipStream_t stream);

// Leaf ids of a group-major walk back to file tree order: out[r * L + j] = src[r * T + flat_of_file[j]], j < L.
// `src` holds [nrow][T] leaf ids of the device copy's trees 0 .. T-1.
hipError_t launch_group_leaf_gather(const float* src, uint64_t nrow, uint32_t T, const uint32_t* flat_of_file,
                                    uint32_t L, float* out, hipStream_t stream);

// One group's block into a [nrow][G][W] array: out[(r * G + g) * W + k] = src[r * W + k].  A copy: no arithmetic.
hipError_t launch_group_block_scatter(const float* src, uint64_t nrow, uint32_t W, uint32_t G, uint32_t g, float* out,
                                      hipStream_t stream);

}  // namespace ohx
