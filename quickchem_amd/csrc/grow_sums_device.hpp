// What the kernel files of the calls with row weights share (grow_weighted.hip, grow_deep.hip), each written once: a
// row's weight as its fixed-point hessian, one row's hq * e^2 in three 64-bit parts, and the block's reduction of them.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "walk_device.hpp"

namespace ohx {

constexpr unsigned long long kGrowLow32 = 0xFFFFFFFFull;
constexpr int kGrowWaves = (int)kGrowBlock / kWave;

// a row's weight and its fixed-point hessian; false where the weight is out of range
__device__ inline bool grow_row_weight(const float* weights, uint64_t row, float* w, unsigned long long* hq) {
  *w = weights != nullptr ? weights[row] : 1.0f;
  if (!grow_weight_sound(*w)) {
    *hq = 0ull;
    return false;
  }
  *hq = (unsigned long long)__builtin_rintf(*w * kRefitGradScale);   // < 2^32
  return true;
}

// a lane's sums: S in three parts, and W
struct GrowWideAcc {
  unsigned long long p2 = 0, p1 = 0, p0 = 0, w = 0;
};

// one row's hq * e^2 into the lane's accumulators; false where the residual is out of range
__device__ inline bool grow_add_weighted_square(float pred, float label, unsigned long long hq, GrowWideAcc* acc) {
  const float g = pred - label;
  // (a NaN fails the comparison)
  if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) return false;
  const long long e = (long long)__builtin_rintf(g * kRefitGradScale);
  const unsigned long long m = (unsigned long long)(e < 0 ? -e : e);   // <= 2^32 - 256
  const unsigned long long sq = m * m;
  const unsigned long long ha = hq * (sq >> 32), hb = hq * (sq & kGrowLow32);   // hq, a, b < 2^32: neither product overflows
  acc->p2 += ha >> 32;
  acc->p1 += (ha & kGrowLow32) + (hb >> 32);
  acc->p0 += hb & kGrowLow32;
  return true;
}

// the block's sums leave it with one set of global adds: p2, p1, p0 to slot, and W to wslot where there is one
__device__ inline void grow_reduce_wide(GrowWideAcc acc, unsigned long long* slot, unsigned long long* wslot) {
  __shared__ unsigned long long part[kGrowWaves][4];
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    acc.p2 += __shfl_xor(acc.p2, d, kWave);
    acc.p1 += __shfl_xor(acc.p1, d, kWave);
    acc.p0 += __shfl_xor(acc.p0, d, kWave);
    acc.w += __shfl_xor(acc.w, d, kWave);
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    part[wave][0] = acc.p2;
    part[wave][1] = acc.p1;
    part[wave][2] = acc.p0;
    part[wave][3] = acc.w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t[4] = {0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < kGrowWaves; ++w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] += part[w][k];
    }
    atomicAdd(&slot[0], t[0]);
    atomicAdd(&slot[1], t[1]);
    atomicAdd(&slot[2], t[2]);
    if (wslot != nullptr) atomicAdd(wslot, t[3]);
  }
}

}  // namespace ohx
#endif  // __HIPCC__
