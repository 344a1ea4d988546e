// gfx950 kernels of the SHAP interaction values (include/ohxgb.h, OHXBoosterPredictInteractions; host side in
// contribs.cpp, design in docs/12_contributions.md section 12.6).  The contributions phi come first, from
// contribs.hip's launch; what is here only adds the matrix.
//
// Exact mode.  Phi_ik (i != k) = (phi_k | i on - phi_k | i off) / 2, xgboost 1.6.0's conditioning inside TreeSHAP.
// Per path that holds feature i as element c this is
//   1/2 (o_c - z_c) (o_k - z_k) leaf W(path without c, k)
// with W the unwound path sum of the path's other elements: c is left out of the permutation, and "on" / "off" only
// scale the path's weight by o_c / z_c.  One wave owns one (64-row tile, feature i, tree group); one lane one row.  Per
// tree the wave zeroes a [feature][lane] tile for matrix row i in LDS, walks the tree's paths that hold i (the
// feature-path index, by length class), and for each runs contribs.hip's recurrences over the other d - 1 elements,
// unrolled to the class's maximum, with the scale (o_c - z_c) * leaf / 2 per lane.  The tree's row is then added into
// the output in tree order from 0.0f (direct), or stored in `part` and summed in tree order by a second launch
// (split): the same per-tree vectors in the same order either way, so a row's bits do not depend on the shape.
// interactions_finish_kernel then writes the diagonal Phi_ii = phi_i - sum_{k != i} Phi_ik in 1.6.0's order, and the
// bias row and column.  No float atomics.
//
// Approximate mode (1.6.0's approximate walk ignores the condition): only the finishing kernel runs, with every
// off-diagonal 0, so the diagonal is the approximate contributions' vector.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "contribs.hpp"

namespace ohx {

namespace {

constexpr int kWave = (int)kContribsTileRows;

#ifdef __HIP_DEVICE_COMPILE__
typedef const __attribute__((address_space(1))) PathElem* g_elem_ptr;
typedef const __attribute__((address_space(1))) float4* g_coef_ptr;
#else
typedef const PathElem* g_elem_ptr;
typedef const float4* g_coef_ptr;
#endif

__device__ __forceinline__ bool one_fraction(float x, const PathElem& el) {
  return (x != x) ? (el.feat >> 31) != 0u : (!(x < el.lo) && !(x >= el.hi));
}

// The paths p = list[q], q in [q0, q1), all of one length class whose longest path has MAXD elements; each holds
// feature `fi`.  xt / ct: this lane's column of the row tile / of the tree's tile for matrix row fi.
template <int MAXD>
__device__ __forceinline__ void conditioned_paths(const PathHead* __restrict__ heads,
                                                  const PathElem* __restrict__ elems,
                                                  const float4* __restrict__ coef_all,
                                                  const uint32_t* __restrict__ list, uint32_t q0, uint32_t q1,
                                                  uint32_t fi, const float* __restrict__ xt, float* __restrict__ ct) {
  constexpr int R = MAXD - 1;   // the longest path without its conditioning element
  for (uint32_t q = q0; q < q1; ++q) {
    const PathHead h = heads[list[q]];
    if (h.len < 2u) continue;   // i alone on its path: no other feature to interact with
    const uint32_t d = h.len - 1u;
    g_elem_ptr e = (g_elem_ptr)(elems + h.first);
    uint32_t c = 0;
    while (c + 1u < h.len && (e[c].feat & 0x7FFFFFFFu) != fi) ++c;
    const PathElem ec = e[c];
    const float oc = one_fraction(xt[fi * kWave], ec) ? 1.0f : 0.0f;
    const float scale = (oc - ec.z) * (0.5f * h.leaf);
    float pw[R + 1];
    uint32_t omask = 0u;
    pw[0] = 1.0f;
#pragma unroll
    for (int k = 1; k <= R; ++k) {
      pw[k] = 0.0f;
      if ((uint32_t)k <= d) {
        asm volatile("" : "+s"(e));
        const PathElem el = e[(uint32_t)(k - 1) + ((uint32_t)(k - 1) >= c ? 1u : 0u)];
        const bool o = one_fraction(xt[(el.feat & 0x7FFFFFFFu) * kWave], el);
        omask |= (o ? 1u : 0u) << (k - 1);
        const float of = o ? 1.0f : 0.0f;
#pragma unroll
        for (int i = k - 1; i >= 0; --i) {
          pw[i + 1] += of * pw[i] * ((float)(i + 1) / (float)(k + 1));
          pw[i] = el.z * pw[i] * ((float)(k - i) / (float)(k + 1));
        }
      }
    }
    float pwd = 0.0f;
#pragma unroll
    for (int i = 1; i <= R; ++i)
      if ((uint32_t)i == d) pwd = pw[i];
    for (uint32_t k = 1; k <= d; ++k) {
      g_coef_ptr coef = (g_coef_ptr)(coef_all + (size_t)d * kCoefStride);
      asm volatile("" : "+s"(coef));
      const PathElem el = e[(k - 1u) + (k - 1u >= c ? 1u : 0u)];
      const bool o = ((omask >> (k - 1)) & 1u) != 0u;
      const float z = el.z;
      const float zinv = z != 0.0f ? 1.0f / z : 0.0f;
      float nop = pwd, total = 0.0f;
#pragma unroll
      for (int i = R - 1; i >= 0; --i) {
        if ((uint32_t)i < d) {
          if ((i & 7) == 7) asm volatile("" : "+s"(coef));
          const float4 cf = coef[i];
          const float tmp = nop * cf.x;
          nop = pw[i] - tmp * z * cf.y;
          total += o ? tmp : pw[i] * zinv * cf.z;
        }
      }
      ct[(el.feat & 0x7FFFFFFFu) * kWave] += total * ((o ? 1.0f : 0.0f) - z) * scale;
    }
  }
}

// One block = one wave = one (tile, feature) unit (direct) or one (tile, feature, tree group) item (split).
// LDS: two [nfeat][64] float tiles, the row tile and the tree's matrix row.
template <bool SPLIT>
__global__ __launch_bounds__(kWave) void interactions_kernel(InteractionsArgs a, uint64_t tile0,
                                                             uint32_t trees_per_group, uint32_t groups,
                                                             const PathHead* __restrict__ heads,
                                                             const PathElem* __restrict__ elems,
                                                             const uint32_t* __restrict__ fpaths,
                                                             const uint32_t* __restrict__ fstart,
                                                             const float4* __restrict__ coef, float* __restrict__ out,
                                                             float* __restrict__ part) {
  extern __shared__ float lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t F = a.nfeat;
  const uint64_t item = blockIdx.x;
  const uint64_t unit = SPLIT ? item / groups : item;
  const uint32_t g = SPLIT ? (uint32_t)(item % groups) : 0u;
  const uint64_t tile = tile0 + unit / F;
  const uint32_t fi = (uint32_t)(unit % F);
  const uint64_t row = tile * kWave + lane;
  const bool valid = row < a.nrow;
  float* __restrict__ xt = lds + lane;
  float* __restrict__ ct = lds + (size_t)F * kWave + lane;
  const uint32_t t0 = a.tree_begin + g * trees_per_group;
  const uint32_t t1 = SPLIT ? min(t0 + trees_per_group, a.tree_end) : a.tree_end;
  const uint32_t ntree = a.tree_end - a.tree_begin;
  const bool missing_is_nan = a.missing != a.missing;
  const float* __restrict__ x = a.rows + (valid ? row : 0) * (uint64_t)a.ncol;
  const float qnan = __builtin_nanf("");
  for (uint32_t f = 0; f < F; ++f) {
    float v = 0.0f;
    if (valid) {
      v = f < a.ncol ? x[f] : qnan;
      if (!missing_is_nan && v == a.missing) v = qnan;
    }
    xt[f * kWave] = v;
  }
  const uint64_t F1 = (uint64_t)F + 1;
  float* __restrict__ orow = out + (valid ? row : 0) * F1 * F1 + (uint64_t)fi * F1;
  for (uint32_t t = t0; t < t1; ++t) {
    for (uint32_t f = 0; f < F; ++f) ct[f * kWave] = 0.0f;
    const uint32_t* __restrict__ cs = fstart + ((size_t)t * F + fi) * (kPathClasses + 1);
    static_assert(kPathClasses == 7, "one body per length class");
    conditioned_paths<4>(heads, elems, coef, fpaths, cs[0], cs[1], fi, xt, ct);
    conditioned_paths<8>(heads, elems, coef, fpaths, cs[1], cs[2], fi, xt, ct);
    conditioned_paths<12>(heads, elems, coef, fpaths, cs[2], cs[3], fi, xt, ct);
    conditioned_paths<16>(heads, elems, coef, fpaths, cs[3], cs[4], fi, xt, ct);
    conditioned_paths<20>(heads, elems, coef, fpaths, cs[4], cs[5], fi, xt, ct);
    conditioned_paths<24>(heads, elems, coef, fpaths, cs[5], cs[6], fi, xt, ct);
    conditioned_paths<32>(heads, elems, coef, fpaths, cs[6], cs[7], fi, xt, ct);
    if (SPLIT) {
      float* __restrict__ dst = part + (((tile * F + fi) * ntree + (t - a.tree_begin)) * F) * kWave + lane;
      for (uint32_t f = 0; f < F; ++f) dst[(size_t)f * kWave] = ct[f * kWave];
    } else if (valid) {
      for (uint32_t f = 0; f < F; ++f) orow[f] = (t == t0 ? 0.0f : orow[f]) + ct[f * kWave];
    }
  }
  if (!SPLIT && valid && t0 == t1)
    for (uint32_t f = 0; f < F; ++f) orow[f] = 0.0f;
}

// The second launch of a split: one wave per (tile, feature i), out[row][i][k] = ((0 + part[t0][k]) + part[t0+1][k])..
__global__ __launch_bounds__(kWave) void interactions_combine_kernel(InteractionsArgs a,
                                                                     const float* __restrict__ part) {
  const uint32_t lane = threadIdx.x;
  const uint32_t F = a.nfeat;
  const uint64_t tile = blockIdx.x / F;
  const uint32_t fi = blockIdx.x % F;
  const uint64_t row = tile * kWave + lane;
  if (row >= a.nrow) return;
  const uint32_t ntree = a.tree_end - a.tree_begin;
  const uint64_t F1 = (uint64_t)F + 1;
  float* __restrict__ orow = a.out + row * F1 * F1 + (uint64_t)fi * F1;
  const float* __restrict__ src = part + (tile * F + fi) * ntree * F * kWave + lane;
  for (uint32_t f = 0; f < F; ++f) {
    float acc = 0.0f;
    for (uint32_t t = 0; t < ntree; ++t) acc += src[((size_t)t * F + f) * kWave];
    orow[f] = acc;
  }
}

// One thread per (row, matrix row i), i = 0 .. F.  1.6.0's order: the diagonal starts from 0, then for k = 0 .. F
// adds phi_i at k == i and subtracts Phi_ik otherwise.  Row F and column F hold nothing but the diagonal's phi_F.
// APPROX: every off-diagonal is 0 (written here).
template <bool APPROX>
__global__ __launch_bounds__(256) void interactions_finish_kernel(InteractionsArgs a) {
  const uint64_t F1 = (uint64_t)a.nfeat + 1;
  const uint64_t n = a.nrow * F1;
  for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t row = idx / F1;
    const uint64_t i = idx % F1;
    const float* __restrict__ ph = a.phi + row * F1;
    float* __restrict__ o = a.out + row * F1 * F1 + i * F1;
    const bool zero_row = APPROX || i == F1 - 1;   // off-diagonals 0: approximate mode, the bias row
    float diag = 0.0f;
    for (uint64_t k = 0; k < F1; ++k) {
      if (k == i) {
        diag += ph[i];
      } else if (zero_row || k == F1 - 1) {      // ... and the bias column
        o[k] = 0.0f;
        diag -= 0.0f;
      } else {
        diag -= o[k];
      }
    }
    o[i] = diag;
  }
}

}  // namespace

int launch_interactions(bool approximate, const InteractionsArgs& a, const ContribsPlan& plan, float* part,
                        void* stream) {
  if (a.nrow == 0) return (int)hipSuccess;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t F = a.nfeat;
  if (!approximate) {
    const uint64_t tiles = (a.nrow + kWave - 1) / kWave;
    const size_t lds = (size_t)2 * F * kWave * sizeof(float);
    const float4* coef = reinterpret_cast<const float4*>(a.coef);
    if (plan.split) {
      const uint64_t items = tiles * F * plan.groups;
      hipLaunchKernelGGL((interactions_kernel<true>), dim3((unsigned)items), dim3(kWave), lds, s, a, (uint64_t)0,
                         plan.trees_per_group, plan.groups, a.heads, a.elems, a.fpaths, a.fstart, coef, a.out, part);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(interactions_combine_kernel, dim3((unsigned)(tiles * F)), dim3(kWave), 0, s, a,
                         (const float*)part);
      e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    } else {
      const uint64_t chunk = interactions_tiles_per_launch(F);
      for (uint64_t t = 0; t < tiles; t += chunk) {
        const uint64_t n = tiles - t < chunk ? tiles - t : chunk;
        hipLaunchKernelGGL((interactions_kernel<false>), dim3((unsigned)(n * F)), dim3(kWave), lds, s, a, t, 0u, 1u,
                           a.heads, a.elems, a.fpaths, a.fstart, coef, a.out, (float*)nullptr);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
      }
    }
  }
  const uint64_t threads = a.nrow * ((uint64_t)F + 1);
  uint64_t blocks = (threads + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (approximate)
    hipLaunchKernelGGL(interactions_finish_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(interactions_finish_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace ohx
