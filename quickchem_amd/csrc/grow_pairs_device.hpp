// What the kernels of the pair path share (grow_pairs.hip; design in docs/26_objectives.md), each written once: the planes
// and the list as a kernel takes them, a row's pair as the histogram kernels read it, and a block's features packed four
// to a wave-uniform word.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "walk_device.hpp"

namespace ohx {

// The pair planes of the round at hand and the histogram columns of the tree at hand: column k is feature list[k]
// (ascending; the identity list where the call samples no columns).
struct GrowPairPlanes {
  long long* q = nullptr;          // [nrow] int64: rint(g * w * 2^24)
  uint32_t* hq = nullptr;          // [nrow] rint(h * w * 2^24)
  const uint8_t* list = nullptr;   // [ncols]
  uint32_t ncols = 0;
  float slope = 1.0f;
};

// A row's pair as two's-complement words, ready for the 64-bit integer adds; false where it is (0, 0): a row out of the
// bag, a row that raised a flag, or a row with nothing to add.
__device__ inline bool grow_load_pair(const GrowPairPlanes& p, uint64_t row, unsigned long long* q, unsigned long long* hq) {
  *hq = (unsigned long long)p.hq[row];
  *q = (unsigned long long)p.q[row];
  return (*q | *hq) != 0ull;
}

// Bit `row & 63` of the bag's plane, read by one scalar load a wave: a wave's 64 rows share one word wherever a block's
// first row and the grid's stride are multiples of 64 (rows < 2^31, so the word index fits 32 bits).  The plane is written
// before the kernel starts and by nothing while it runs; the constant address space says so.
typedef const unsigned long long __attribute__((address_space(4))) * GrowBagWords;
__device__ inline bool grow_row_in_bag(const unsigned long long* bag, uint64_t row) {
  const uint32_t word = __builtin_amdgcn_readfirstlane((uint32_t)(row >> 6));
  const unsigned long long bits = ((GrowBagWords)bag)[word];
  return ((bits >> (row & 63u)) & 1ull) != 0ull;
}

// nf features of `feat` (nf <= 4 * WORDS), a byte each in wave-uniform words, so that a row loop forms a bin plane's
// address with scalar arithmetic.  A byte past the last feature repeats its word's first feature: a load through it reads
// an address that the word's first load reads, and is not used.
template <uint32_t WORDS>
__device__ inline void grow_pack_features(const uint8_t* feat, uint32_t nf, uint32_t (&pack)[WORDS]) {
#pragma unroll
  for (uint32_t j = 0; j < WORDS; ++j) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
      if (4 * j < nf) v |= (uint32_t)feat[4 * j + b < nf ? 4 * j + b : 4 * j] << (8 * b);
    pack[j] = __builtin_amdgcn_readfirstlane(v);
  }
}

}  // namespace ohx
#endif  // __HIPCC__
