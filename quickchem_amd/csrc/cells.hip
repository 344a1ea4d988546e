// Kernels of the selected-gridcells calls (cells.hpp; include/ohxgb.h part 2b; docs/15_selected_cells.md).
//
// Selection and scatter are ORDERED passes over a list cut into at most kCellsMaxBlocks contiguous chunks
// (plan_cells_pass): a first launch leaves one number per block in `table` (how many cells the block selects; the
// greatest entry of the block's part of the list), the second launch has every block reduce the entries of the blocks
// in front of it - its offset, or the running maximum it starts from - and then walks its chunk 256 items at a time,
// ordering the four waves of a step through LDS.  Positions come from these sums alone: no atomic counter, the same
// array every run.  The only atomics are integer ORs on the caller's status word.
//
// The gather gives a wave 64 consecutive entries of `cells`, one cell per lane.  Each field's load puts neighbouring
// cells on neighbouring addresses; the values go to LDS as [lane][nfield] with the lane stride made odd, and the
// wave's 64 rows - one contiguous run of 64 * nfield floats of `rows` - are stored 64 consecutive floats per
// instruction.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cells.hpp"

namespace ohx {
namespace {

constexpr uint32_t kWavesPerBlock = kCellsBlock / kCellsWave;

__device__ inline uint32_t lane_rank(uint64_t mask) {       // set bits of `mask` below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline long long wave_max(long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const long long u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}
__device__ inline uint32_t wave_or(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}

// ---- selection ----

// Box cell q (i fastest, then j, then k) -> its cell index; whether it is selected.  `small`: the box has fewer than
// 2^32 cells (wave-uniform), so the divisions are 32-bit.
__device__ inline bool box_cell_selected(const SelectCellsArgs& s, uint64_t q, bool small, int64_t* cell) {
  uint64_t bi, bj, bk;
  if (small) {
    const uint32_t q32 = (uint32_t)q, wi = (uint32_t)s.wi, wj = (uint32_t)s.wj;
    const uint32_t t = q32 / wi;
    bi = q32 - t * wi;
    bk = t / wj;
    bj = t - (uint32_t)bk * wj;
  } else {
    const uint64_t t = q / (uint64_t)s.wi;
    bi = q - t * (uint64_t)s.wi;
    bk = t / (uint64_t)s.wj;
    bj = t - bk * (uint64_t)s.wj;
  }
  const int64_t c2 = (s.i0 + (int64_t)bi) + s.im * (s.j0 + (int64_t)bj);
  const int64_t c = c2 + s.im * s.jm * (s.k0 + (int64_t)bk);
  *cell = c;
  if (s.a == nullptr) return true;
  const float av = s.a[s.a_is2d ? c2 : c];
  const float bv = s.b != nullptr ? s.b[s.b_is2d ? c2 : c] : s.b0;
  return av > bv;       // false when either side is NaN
}

// First launch: table[block] = selected cells of the block's chunk.
__global__ __launch_bounds__(kCellsBlock) void select_count_kernel(SelectCellsArgs s, uint64_t nbox, uint64_t chunk,
                                                                   uint64_t* __restrict__ table) {
  __shared__ uint64_t wave_count[kWavesPerBlock];
  const uint32_t tid = threadIdx.x, wave = tid / kCellsWave;
  const bool small = nbox <= 0xFFFFFFFFull;
  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  const uint64_t end = begin + chunk < nbox ? begin + chunk : nbox;
  uint64_t n = 0;      // wave-uniform
  for (uint64_t q0 = begin; q0 < end; q0 += kCellsBlock) {
    const uint64_t q = q0 + tid;
    int64_t c;
    const bool sel = q < end && box_cell_selected(s, q, small, &c);
    n += (uint64_t)__popcll(__ballot(sel));
  }
  if (tid % kCellsWave == 0) wave_count[wave] = n;
  __syncthreads();
  if (tid == 0) {
    uint64_t total = 0;
    for (uint32_t w = 0; w < kWavesPerBlock; ++w) total += wave_count[w];
    table[blockIdx.x] = total;
  }
}

// Second launch: the block's offset is the sum of the counts in front of it; its cells follow in box order.
__global__ __launch_bounds__(kCellsBlock) void select_write_kernel(SelectCellsArgs s, uint64_t nbox, uint64_t chunk,
                                                                   const uint64_t* __restrict__ table,
                                                                   int64_t* __restrict__ cells,
                                                                   int64_t* __restrict__ count,
                                                                   uint32_t* __restrict__ status) {
  __shared__ unsigned long long front[kWavesPerBlock];
  __shared__ uint32_t wave_count[kWavesPerBlock];
  const uint32_t tid = threadIdx.x, wave = tid / kCellsWave;
  const bool small = nbox <= 0xFFFFFFFFull;
  unsigned long long part = 0;
  for (uint32_t t = tid; t < blockIdx.x; t += kCellsBlock) part += table[t];
  part = wave_sum(part);
  if (tid % kCellsWave == 0) front[wave] = part;
  __syncthreads();
  uint64_t base = 0;
  for (uint32_t w = 0; w < kWavesPerBlock; ++w) base += front[w];
  const uint64_t cap = (uint64_t)s.cap;
  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  const uint64_t end = begin + chunk < nbox ? begin + chunk : nbox;
  for (uint64_t q0 = begin; q0 < end; q0 += kCellsBlock) {
    const uint64_t q = q0 + tid;
    int64_t c = 0;
    const bool sel = q < end && box_cell_selected(s, q, small, &c);
    const uint64_t mask = __ballot(sel);
    if (tid % kCellsWave == 0) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, step = 0;
    for (uint32_t w = 0; w < kWavesPerBlock; ++w) {
      before += w < wave ? wave_count[w] : 0u;
      step += wave_count[w];
    }
    const uint64_t pos = base + before + lane_rank(mask);
    if (sel && pos < cap) cells[pos] = c;
    base += step;
    __syncthreads();
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    *count = (int64_t)base;
    if (base > cap && status != nullptr) atomicOr(status, kCellsOverCap);
  }
}

// ---- gather ----

__global__ __launch_bounds__(kCellsWave) void gather_cells_kernel(GatherCellsArgs g, uint64_t tile0,
                                                                  const int64_t* __restrict__ cells, int64_t ncell,
                                                                  float* __restrict__ rows,
                                                                  uint32_t* __restrict__ status) {
  extern __shared__ float tile[];      // [64][stride]
  const uint32_t lane = threadIdx.x;
  const uint32_t nfield = g.nfield, stride = nfield | 1u;
  const int64_t n0 = (int64_t)((tile0 + blockIdx.x) * kCellsWave);
  const int64_t n = n0 + lane;
  const bool have = n < ncell;
  const int64_t c = have ? cells[n] : 0;
  const bool in_range = have && c >= 0 && c < g.ncells_total;      // a cell out of range is never dereferenced
  const int64_t at3 = in_range ? c : 0;
  int64_t at2 = 0;
  if (in_range) at2 = g.ncells_total <= 0xFFFFFFFFll ? (int64_t)((uint32_t)c % (uint32_t)g.plane) : c % g.plane;
  float* __restrict__ mine = tile + lane * stride;
  // eight fields' loads are issued before the first of them is waited for
  constexpr uint32_t kBatch = 8;
  for (uint32_t f0 = 0; f0 < nfield; f0 += kBatch) {
    float v[kBatch];
#pragma unroll
    for (uint32_t b = 0; b < kBatch; ++b) {
      const uint32_t f = f0 + b;
      v[b] = __builtin_nanf("");
      if (in_range && f < nfield) {
        const float* __restrict__ src = g.field[f];
        v[b] = src[((g.is2d_mask >> f) & 1u) ? at2 : at3];
      }
    }
#pragma unroll
    for (uint32_t b = 0; b < kBatch; ++b) {
      const uint32_t f = f0 + b;
      if (f >= nfield) break;
      if (f == g.pl_feature) {
        asm volatile("");      // a branch, taken for one field, not a division computed for all and selected
        v[b] = v[b] / 100.0f;
      }
      mine[f] = v[b];
    }
  }
  if (status != nullptr && __ballot(have && !in_range) != 0 && lane == 0) atomicOr(status, kCellsOutOfRange);
  __syncthreads();
  // the wave's rows are floats [n0 * nfield, (n0 + rows_here) * nfield) of `rows`: 64 consecutive ones per store
  const int64_t left = ncell - n0;
  const uint32_t rows_here = left < (int64_t)kCellsWave ? (uint32_t)left : kCellsWave;
  const uint32_t total = rows_here * nfield;
  float* __restrict__ dst = rows + n0 * (int64_t)nfield;
  const uint32_t row_step = kCellsWave / nfield, col_step = kCellsWave % nfield;
  uint32_t r = lane / nfield, f = lane % nfield;
  for (uint32_t e = lane; e < total; e += kCellsWave) {
    dst[e] = tile[r * stride + f];
    r += row_step;
    f += col_step;
    if (f >= nfield) {
      f -= nfield;
      r += 1;
    }
  }
}

// ---- scatter ----

constexpr long long kLowest = (long long)0x8000000000000000ull;

// First launch: table[block] = the greatest entry of the block's chunk of `cells`.
__global__ __launch_bounds__(kCellsBlock) void scatter_max_kernel(const int64_t* __restrict__ cells, uint64_t ncell,
                                                                  uint64_t chunk, uint64_t* __restrict__ table) {
  __shared__ long long wave_top[kWavesPerBlock];
  const uint32_t tid = threadIdx.x, wave = tid / kCellsWave;
  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  const uint64_t end = begin + chunk < ncell ? begin + chunk : ncell;
  long long top = kLowest;
  for (uint64_t n = begin + tid; n < end; n += kCellsBlock) {
    const long long c = cells[n];
    top = c > top ? c : top;
  }
  top = wave_max(top);
  if (tid % kCellsWave == 0) wave_top[wave] = top;
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < kWavesPerBlock; ++w) top = wave_top[w] > top ? wave_top[w] : top;
    table[blockIdx.x] = (uint64_t)top;
  }
}

// Second launch: entry n is stored when its cell is in range and above every entry in front of it - for a strictly
// ascending list, every entry.  So no cell is stored twice, whatever the list holds.
__global__ __launch_bounds__(kCellsBlock) void scatter_write_kernel(const float* __restrict__ values, int64_t stride,
                                                                    int64_t col, const int64_t* __restrict__ cells,
                                                                    uint64_t ncell, uint64_t chunk,
                                                                    const uint64_t* __restrict__ table,
                                                                    float* __restrict__ out3d, int64_t ncells_total,
                                                                    uint32_t* __restrict__ status) {
  __shared__ long long wave_top[kWavesPerBlock];
  const uint32_t tid = threadIdx.x, wave = tid / kCellsWave, lane = tid % kCellsWave;
  long long top = kLowest;
  for (uint32_t t = tid; t < blockIdx.x; t += kCellsBlock) {
    const long long m = (long long)table[t];
    top = m > top ? m : top;
  }
  top = wave_max(top);
  if (lane == 0) wave_top[wave] = top;
  __syncthreads();
  long long base = kLowest;      // the greatest entry in front of this step
  for (uint32_t w = 0; w < kWavesPerBlock; ++w) base = wave_top[w] > base ? wave_top[w] : base;
  __syncthreads();
  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  const uint64_t end = begin + chunk < ncell ? begin + chunk : ncell;
  uint32_t bits = 0;
  for (uint64_t n0 = begin; n0 < end; n0 += kCellsBlock) {
    const uint64_t n = n0 + tid;
    const bool have = n < end;
    const long long c = have ? cells[n] : kLowest;
    long long incl = c;      // greatest entry of lanes 0 .. lane of this wave
    for (uint32_t o = 1; o < kCellsWave; o <<= 1) {
      const long long u = __shfl_up(incl, o);
      if (lane >= o && u > incl) incl = u;
    }
    long long before = __shfl_up(incl, 1u);
    if (lane == 0) before = kLowest;
    if (lane == kCellsWave - 1) wave_top[wave] = incl;
    __syncthreads();
    long long step = base;
    for (uint32_t w = 0; w < kWavesPerBlock; ++w) {
      const long long m = wave_top[w];
      if (w < wave && m > before) before = m;
      if (m > step) step = m;
    }
    if (base > before) before = base;
    if (have) {
      const bool in_range = c >= 0 && c < ncells_total;
      const bool above = c > before;
      if (!in_range) bits |= kCellsOutOfRange;
      if (!above) bits |= kCellsNotAscending;
      if (in_range && above) out3d[c] = values[(int64_t)n * stride + col];
    }
    base = step;
    __syncthreads();
  }
  bits = wave_or(bits);
  if (status != nullptr && bits != 0 && lane == 0) atomicOr(status, bits);
}

}  // namespace

int launch_select_cells(const SelectCellsArgs& a, uint64_t* table, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t nbox = (uint64_t)a.wi * (uint64_t)a.wj * (uint64_t)a.wk;
  const CellsPassPlan p = plan_cells_pass(nbox);
  if (p.blocks == 0) return (int)hipMemsetAsync(a.count, 0, sizeof(int64_t), s);
  hipLaunchKernelGGL(select_count_kernel, dim3(p.blocks), dim3(kCellsBlock), 0, s, a, nbox, p.chunk, table);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(select_write_kernel, dim3(p.blocks), dim3(kCellsBlock), 0, s, a, nbox, p.chunk,
                     (const uint64_t*)table, a.cells, a.count, a.status);
  return (int)hipGetLastError();
}

int launch_gather_cells(const GatherCellsArgs& g, const int64_t* cells, int64_t ncell, float* rows, uint32_t* status,
                        void* stream) {
  if (ncell <= 0) return (int)hipSuccess;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t tiles = ((uint64_t)ncell + kCellsWave - 1) / kCellsWave;
  const size_t lds = (size_t)kCellsWave * cells_gather_lds_stride(g.nfield) * sizeof(float);
  const uint64_t per_launch = 1ull << 24;
  for (uint64_t t = 0; t < tiles; t += per_launch) {
    const uint64_t n = tiles - t < per_launch ? tiles - t : per_launch;
    hipLaunchKernelGGL(gather_cells_kernel, dim3((unsigned)n), dim3(kCellsWave), lds, s, g, t, cells, ncell, rows,
                       status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return (int)hipSuccess;
}

int launch_scatter_cells(const float* values, int64_t stride, int64_t col, const int64_t* cells, int64_t ncell,
                         float* out3d, int64_t ncells_total, uint32_t* status, uint64_t* table, void* stream) {
  if (ncell <= 0) return (int)hipSuccess;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CellsPassPlan p = plan_cells_pass((uint64_t)ncell);
  hipLaunchKernelGGL(scatter_max_kernel, dim3(p.blocks), dim3(kCellsBlock), 0, s, cells, (uint64_t)ncell, p.chunk,
                     table);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(scatter_write_kernel, dim3(p.blocks), dim3(kCellsBlock), 0, s, values, stride, col, cells,
                     (uint64_t)ncell, p.chunk, (const uint64_t*)table, out3d, ncells_total, status);
  return (int)hipGetLastError();
}

}  // namespace ohx
