// gfx950 kernels of the device quantile cuts (cuts.hpp; design in docs/19_device_cuts.md).
//
//   cuts_hist_kernel<1>    a lane takes a sampled row and walks the columns of its block's group: the top 12 key bits of
//                          every kept value are counted in block-private LDS histograms (4096 counters a column), and
//                          the block flushes its nonzero counters once with global integer adds.
//   cuts_hist_kernel<2|3>  the columns' selected prefixes are staged in LDS; a lane finds its value's slot by binary
//                          search and counts the next 10 key bits in the global table [column][slot][1024].
//   cuts_select_kernel<P>  after pass P, one block per column:     every target steps to the digit that holds its rank,
//                          the alive rule is applied, and the next selection is written - the arithmetic of cuts.hpp,
//                          which the host build runs too.
// A wave whose counting lanes all hit one counter makes one add of the lane count (a constant or mostly-zero column).
// Only integer adds: no float atomics, no compare-and-swap loops, and the same cuts whatever the order of the rows or the
// launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cuts.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kCutsBlock;
constexpr int kSelectBlock = (int)kCutsSelectBlock;

// Adds one to base[idx] for every lane with `valid`; the whole wave must be here.
__device__ inline void wave_count(uint32_t* base, uint32_t idx, bool valid) {
  const unsigned long long mask = __ballot(valid);
  if (mask == 0ull) return;
  const int leader = __ffsll((long long)mask) - 1;
  const uint32_t first = __shfl(idx, leader, kWave);
  const unsigned long long same = __ballot(valid && idx == first);
  if (same == mask) {
    if ((int)(threadIdx.x & (kWave - 1)) == leader) atomicAdd(base + first, (uint32_t)__popcll(mask));
  } else if (valid) {
    atomicAdd(base + idx, 1u);
  }
}

// grid (blocks over the sampled rows, column groups); dynamic LDS: PASS 1 col_group x 4096 counters, else the group's
// staged prefixes, col_group x 255
template <int PASS>
__global__ __launch_bounds__(kBlock) void cuts_hist_kernel(CutsArgs a, uint32_t col_group) {
  extern __shared__ uint32_t cuts_lds[];
  __shared__ uint32_t nsel_s[kCutsMaxGroup];
  const uint32_t c0 = blockIdx.y * col_group;
  if (c0 >= a.ncol) return;
  const uint32_t nc = a.ncol - c0 < col_group ? a.ncol - c0 : col_group;
  if (PASS == 1) {
    for (uint32_t i = threadIdx.x; i < nc * kCutsDigits1; i += kBlock) cuts_lds[i] = 0u;
  } else {
    for (uint32_t i = threadIdx.x; i < nc * kCutsSelStride; i += kBlock) {
      const CutsCol& col = a.cols[c0 + i / kCutsSelStride];
      const uint32_t j = i % kCutsSelStride;
      cuts_lds[i] = j < col.nsel ? col.sel[j] : 0u;
    }
    if (threadIdx.x < nc) {
      const uint32_t n = a.cols[c0 + threadIdx.x].nsel;
      nsel_s[threadIdx.x] = n < kCutsSelStride ? n : kCutsSelStride;
    }
  }
  __syncthreads();
  const bool missing_is_nan = a.missing != a.missing;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  // (the trip count is the block's: every wave reaches wave_count whole)
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < a.sampled; base += stride) {
    const uint64_t s = base + threadIdx.x;
    const bool in = s < a.sampled;
    const float* x = a.rows + (in ? s * a.row_step : 0ull) * (uint64_t)a.ncol + c0;
    for (uint32_t k = 0; k < nc; ++k) {
      const float v = in ? x[k] : 0.0f;
      bool keep = in && cuts_keep(v, a.missing, missing_is_nan);
      const uint32_t key = cuts_key(cuts_float_bits(v));
      if (PASS == 1) {
        wave_count(cuts_lds + k * kCutsDigits1, key >> (32 - kCutsBits1), keep);
      } else {
        const uint32_t prefix = PASS == 2 ? key >> (32 - kCutsBits1) : key >> kCutsBits3;
        const uint32_t digit = PASS == 2 ? (key >> kCutsBits3) & (kCutsDigits - 1) : key & (kCutsDigits - 1);
        const uint32_t nsel = nsel_s[k];
        const uint32_t slot = cuts_find_slot(cuts_lds + k * kCutsSelStride, nsel, prefix);
        keep = keep && slot < nsel;
        wave_count(a.table + (uint64_t)(c0 + k) * (kCutsMaxBins * kCutsDigits), slot * kCutsDigits + digit, keep);
      }
    }
  }
  if (PASS == 1) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nc * kCutsDigits1; i += kBlock) {
      const uint32_t v = cuts_lds[i];
      if (v != 0u) atomicAdd(&a.table1[(uint64_t)c0 * kCutsDigits1 + i], v);
    }
  }
}

// exclusive sums of v over the block's threads, and their total; buf: kSelectBlock words of LDS
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* buf, uint32_t* total) {
  const uint32_t t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < (uint32_t)kSelectBlock; d <<= 1) {
    const uint32_t x = t >= d ? buf[t - d] : 0u;
    __syncthreads();
    buf[t] += x;
    __syncthreads();
  }
  const uint32_t inclusive = buf[t];
  *total = buf[kSelectBlock - 1];
  __syncthreads();
  return inclusive - v;
}

// grid (columns).  PASS 1, 2 or 3: the pass just counted
template <int PASS>
__global__ __launch_bounds__(kSelectBlock) void cuts_select_kernel(CutsArgs a) {
  constexpr uint32_t pass = PASS;
  __shared__ uint32_t row1[PASS == 1 ? kCutsDigits1 : 1];      // pass 1: the column's 4096 counters
  __shared__ uint32_t sel_old[kCutsSlots], sel_new[kCutsSlots], prefix[kCutsSlots], scan[kCutsSlots];
  const uint32_t t = threadIdx.x, c = blockIdx.x, mb = a.max_bins;
  CutsCol& col = a.cols[c];
  const uint32_t bits = pass == 1 ? kCutsBits1 : kCutsBits2, D = 1u << bits;
  const uint32_t* tab = a.table + (uint64_t)c * (kCutsMaxBins * kCutsDigits);
  uint32_t n, nsel, alive_old, slot = 0, rank = 0;
  if (pass == 1) {
    uint32_t sum = 0;
    for (uint32_t i = t; i < kCutsDigits1; i += kSelectBlock) {
      const uint32_t v = a.table1[(uint64_t)c * kCutsDigits1 + i];
      row1[i] = v;
      sum += v;
    }
    (void)block_scan(sum, scan, &n);
    nsel = 1;
    alive_old = 1;
    sel_old[t] = 0u;
    rank = cuts_target_rank(t < mb ? t : 0u, n, mb);
  } else {
    n = col.n;
    nsel = col.nsel < kCutsMaxBins ? col.nsel : kCutsMaxBins;
    alive_old = col.alive;
    sel_old[t] = t < nsel ? col.sel[t] : 0u;
    slot = col.tslot[t];
    rank = col.trank[t];
  }
  __syncthreads();
  // every target steps to the digit that holds its rank
  const bool target = n != 0u && t < mb;
  bool bad = false;
  if (target) {
    uint32_t d = D;
    if (slot < nsel) {
      if (PASS == 1) d = cuts_locate(row1, D, &rank);
      else d = cuts_locate(tab + slot * D, D, &rank);
    }
    if (d == D) {
      bad = true;
      d = D - 1;
    }
    prefix[t] = (sel_old[slot < nsel ? slot : 0u] << bits) | d;
  }
  // the nonzero counters of a contiguous share each, in order
  const uint32_t E = nsel * D, per = (E + kSelectBlock - 1) / kSelectBlock;
  const uint32_t e0 = t * per < E ? t * per : E, e1 = e0 + per < E ? e0 + per : E;
  uint32_t cnt = 0;
  if (alive_old) {
    if (pass == 1) {
      for (uint32_t e = e0; e < e1; ++e) cnt += row1[e] != 0u ? 1u : 0u;
    } else {
      for (uint32_t e = e0; e < e1; ++e) cnt += tab[e] != 0u ? 1u : 0u;
    }
  }
  uint32_t nonzero, k;
  uint32_t at = block_scan(cnt, scan, &nonzero);
  const bool alive = cuts_alive_after(alive_old != 0u, nonzero, mb);
  if (alive) {
    // the next selection is every prefix seen: nonzero <= max_bins of them
    k = nonzero;
    for (uint32_t e = e0; e < e1; ++e) {
      uint32_t v;
      if (PASS == 1) v = row1[e];
      else v = tab[e];
      if (v != 0u && at < kCutsSlots) sel_new[at++] = (sel_old[e / D] << bits) | (e % D);
    }
  } else {
    // the targets' own prefixes, which ascend with the target: duplicates are neighbours
    const bool head = target && (t == 0u || prefix[t] != prefix[t - 1]);
    at = block_scan(head ? 1u : 0u, scan, &k);
    if (head) sel_new[at] = prefix[t];
  }
  __syncthreads();
  if (target) {
    const uint32_t s = cuts_find_slot(sel_new, k, prefix[t]);
    bad = bad || s >= k;
    col.tslot[t] = s;
    col.trank[t] = rank;
  }
  if (t < k) col.sel[t] = sel_new[t];
  if (bad) atomicOr(&col.error, 1u);
  if (t == 0) {
    if (pass == 1) col.n = n;
    col.nsel = k;
    col.alive = alive ? 1u : 0u;
  }
}

}  // namespace

int prepare_cuts() {
  hipError_t e = raise_lds_limit(cuts_hist_kernel<1>, kCutsMaxGroup1 * kCutsDigits1 * sizeof(uint32_t));
  if (e != hipSuccess) return e;
  e = raise_lds_limit(cuts_hist_kernel<2>, kCutsMaxGroup * kCutsSelStride * sizeof(uint32_t));
  if (e != hipSuccess) return e;
  return raise_lds_limit(cuts_hist_kernel<3>, kCutsMaxGroup * kCutsSelStride * sizeof(uint32_t));
}

int launch_cuts(const CutsArgs& a, const CutsPlan& p, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (a.sampled == 0 || a.sampled > kCutsMaxRows || a.sampled != p.sampled || a.row_step < 1 || a.ncol == 0 ||
      a.max_bins < 2 || a.max_bins > kCutsMaxBins || p.blocks1 == 0 || p.blocks == 0 || p.col_group1 == 0 ||
      p.col_group1 > kCutsMaxGroup1 || (uint64_t)p.col_groups1 * p.col_group1 < a.ncol || p.col_group == 0 ||
      p.col_group > kCutsMaxGroup || (uint64_t)p.col_groups * p.col_group < a.ncol ||
      p.lds1_bytes != p.col_group1 * kCutsDigits1 * sizeof(uint32_t) ||
      p.lds_bytes != p.col_group * kCutsSelStride * sizeof(uint32_t) || p.col_groups1 > 65535u || p.col_groups > 65535u ||
      p.table1_bytes != (uint64_t)a.ncol * kCutsDigits1 * sizeof(uint32_t) ||
      p.table_bytes != (uint64_t)a.ncol * kCutsMaxBins * kCutsDigits * sizeof(uint32_t))
    return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if ((e = hipMemsetAsync(a.cols, 0, (size_t)a.ncol * sizeof(CutsCol), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.table1, 0, (size_t)p.table1_bytes, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(cuts_hist_kernel<1>, dim3(p.blocks1, p.col_groups1), dim3(kBlock), p.lds1_bytes, stream, a, p.col_group1);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(cuts_select_kernel<1>, dim3(a.ncol), dim3(kSelectBlock), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.table, 0, (size_t)p.table_bytes, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(cuts_hist_kernel<2>, dim3(p.blocks, p.col_groups), dim3(kBlock), p.lds_bytes, stream, a, p.col_group);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(cuts_select_kernel<2>, dim3(a.ncol), dim3(kSelectBlock), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.table, 0, (size_t)p.table_bytes, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(cuts_hist_kernel<3>, dim3(p.blocks, p.col_groups), dim3(kBlock), p.lds_bytes, stream, a, p.col_group);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(cuts_select_kernel<3>, dim3(a.ncol), dim3(kSelectBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace ohx
