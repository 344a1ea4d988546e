// gfx950 kernels of the per-feature contributions (include/ohxgb.h, OHXBoosterPredictContribs; host side in
// contribs.cpp, design in docs/12_contributions.md).  Separate from kernels.hip: nothing here touches the walk.
//
// Shape.  One lane owns one row; a block is one wave of 64 rows.  Per tree the wave zeroes a contribution tile in
// LDS, feature-major [feature][lane] (every lane only ever touches its own column, so the order of additions is
// fixed), fills it, and adds it into the row's totals - xgboost 1.6.0's this_tree_contribs -> p_contribs.
//
// Exact mode (path-dependent TreeSHAP, Lundberg et al. 2020 Algorithm 2, restated per path): the whole wave is on the
// same path at the same time, so the path's header and elements are wave-uniform and come through scalar loads, and
// the only per-lane data are the row's feature values (a row tile in LDS, the second [feature][lane] tile) and the one
// fractions they imply.  The path weights run in VGPRs, the extend recurrence fully unrolled to the length class's
// maximum (contribs.hpp kPathClassMax; the branches on the path's length are wave-uniform), so no register array is
// indexed at run time.  Then every element's unwound sum, and sum * (o - z) * leaf into the tree's tile.  Totals: the
// lane's own row of the output, read back and written per tree.
//
// Approximate mode (1.6.0 CalculateContributionsApprox): one lane walks its row down each tree, node means beside the
// splits (ContribNode), mean(next) - mean(current) into the split feature's slot of the tree's tile.  Rows are read
// straight from global memory (as predict_rows_direct_kernel does); the totals are the second LDS tile.
//
// Launch shapes (ContribsPlan): direct (a wave walks every tree of its tile) or split (a wave walks a group of trees
// and stores each tree's tile in `part`; contribs_combine_kernel sums them in tree order).  Both add the same per-tree
// vectors in the same order from 0.0f: a row's bits do not depend on the shape.  No float atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "contribs.hpp"

namespace ohx {

namespace {

constexpr int kWave = (int)kContribsTileRows;

__device__ __forceinline__ bool is_inf(float v) { return __builtin_isinf(v); }

// pointers KNOWN to point into global memory: the empty asm statements below, which keep loads from being hoisted, make
// the compiler lose track of a generic pointer's origin, and it would then load through flat instructions
#ifdef __HIP_DEVICE_COMPILE__
typedef const __attribute__((address_space(1))) PathElem* g_elem_ptr;
typedef const __attribute__((address_space(1))) float4* g_coef_ptr;
#else
typedef const PathElem* g_elem_ptr;
typedef const float4* g_coef_ptr;
#endif

// Extend the path by its elements, then add each element's share into the tree's tile.  `xt` / `ct`: this lane's
// column of the row tile / the tree's contribution tile.
// The tables come in as __restrict__ kernel arguments: only then can the compiler prove that the kernel's stores do
// not reach them, and load them through the scalar cache.
template <int MAXD>
__device__ __forceinline__ void shap_paths(const PathHead* __restrict__ heads, const PathElem* __restrict__ elems,
                                           const float4* __restrict__ coef_all, uint32_t p0, uint32_t p1,
                                           const float* __restrict__ xt, float* __restrict__ ct) {
  for (uint32_t p = p0; p < p1; ++p) {
    const PathHead h = heads[p];
    const uint32_t d = h.len;
    g_elem_ptr e = (g_elem_ptr)(elems + h.first);
    float pw[MAXD + 1];
    uint32_t omask = 0u;
    pw[0] = 1.0f;                         // the bias element: z = o = 1
#pragma unroll
    for (int k = 1; k <= MAXD; ++k) {
      pw[k] = 0.0f;
      if ((uint32_t)k <= d) {
        // one element at a time: loaded all at once, MAXD elements would take 4 * MAXD SGPRs and spill
        asm volatile("" : "+s"(e));
        const PathElem el = e[k - 1];
        const float x = xt[(el.feat & 0x7FFFFFFFu) * kWave];
        const bool o = (x != x) ? (el.feat >> 31) != 0u : (!(x < el.lo) && !(x >= el.hi));
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
    for (int i = 1; i <= MAXD; ++i)
      if ((uint32_t)i == d) pwd = pw[i];
    for (uint32_t k = 1; k <= d; ++k) {
      // re-read per element: hoisted out of this loop, the row of coefficients would take 4 * MAXD SGPRs and spill
      g_coef_ptr coef = (g_coef_ptr)(coef_all + (size_t)d * kCoefStride);
      asm volatile("" : "+s"(coef));
      const PathElem el = e[k - 1];
      const bool o = ((omask >> (k - 1)) & 1u) != 0u;
      const float z = el.z;
      const float zinv = z != 0.0f ? 1.0f / z : 0.0f;
      float nop = pwd, total = 0.0f;
#pragma unroll
      for (int i = MAXD - 1; i >= 0; --i) {
        if ((uint32_t)i < d) {
          if ((i & 7) == 7) asm volatile("" : "+s"(coef));   // at most 8 rows of coefficients in SGPRs at a time
          const float4 c = coef[i];
          const float tmp = nop * c.x;
          nop = pw[i] - tmp * z * c.y;
          total += o ? tmp : pw[i] * zinv * c.z;
        }
      }
      ct[(el.feat & 0x7FFFFFFFu) * kWave] += total * ((o ? 1.0f : 0.0f) - z) * h.leaf;
    }
  }
}

__device__ __forceinline__ void exact_tree(const PathHead* __restrict__ heads, const PathElem* __restrict__ elems,
                                           const uint32_t* __restrict__ class_start, const float4* __restrict__ coef,
                                           uint32_t t, const float* __restrict__ xt, float* __restrict__ ct) {
  const uint32_t* __restrict__ cs = class_start + (size_t)t * (kPathClasses + 1);
  static_assert(kPathClasses == 7, "one body per length class");
  shap_paths<4>(heads, elems, coef, cs[0], cs[1], xt, ct);
  shap_paths<8>(heads, elems, coef, cs[1], cs[2], xt, ct);
  shap_paths<12>(heads, elems, coef, cs[2], cs[3], xt, ct);
  shap_paths<16>(heads, elems, coef, cs[3], cs[4], xt, ct);
  shap_paths<20>(heads, elems, coef, cs[4], cs[5], xt, ct);
  shap_paths<24>(heads, elems, coef, cs[5], cs[6], xt, ct);
  shap_paths<32>(heads, elems, coef, cs[6], cs[7], xt, ct);
}

// The row's value of feature f is x[f * STRIDE]: a global row (STRIDE 1) or this lane's column of a row tile in LDS
// (STRIDE kWave, `missing` already NaN there).  Features at or past `ncol` are missing.
template <uint32_t STRIDE>
__device__ __forceinline__ void approx_tree(const ContribsArgs& a, uint32_t t, const float* __restrict__ x,
                                            uint32_t ncol, bool missing_is_nan, float* __restrict__ ct) {
  const uint4* __restrict__ nodes = reinterpret_cast<const uint4*>(a.nodes);
  uint4 nd = nodes[a.roots[t]];
  if (nd.y == 0u) return;
  float cur = __uint_as_float(nd.w);
  uint32_t f = 0u;
  while (nd.y != 0u) {
    f = nd.z & 0x7FFFFFFFu;
    bool miss = true, lt = false;
    if (f < ncol) {
      const float v = x[f * STRIDE];
      miss = (v != v) || (!missing_is_nan && v == a.missing);
      lt = v < __uint_as_float(nd.x);
    }
    const bool go_left = miss ? (nd.z >> 31) != 0u : lt;
    nd = nodes[nd.y + (go_left ? 0u : 1u)];
    const float next = __uint_as_float(nd.w);
    ct[f * kWave] += next - cur;
    cur = next;
  }
  ct[f * kWave] += __uint_as_float(nd.x) - cur;
}

// One block = one wave = one tile of 64 rows (direct) or one (tile, tree group) item (split).
// LDS: two [nfeat][64] float tiles.  Exact: row tile, tree tile.  Approximate: totals, tree tile.
template <bool APPROX, bool SPLIT>
__global__ __launch_bounds__(kWave) void contribs_kernel(ContribsArgs a, uint64_t tile0, uint32_t trees_per_group,
                                                         uint32_t groups, const PathHead* __restrict__ heads,
                                                         const PathElem* __restrict__ elems,
                                                         const uint32_t* __restrict__ class_start,
                                                         const float4* __restrict__ coef, float* __restrict__ out,
                                                         float* __restrict__ part) {
  extern __shared__ float lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t F = a.nfeat;
  const uint64_t item = blockIdx.x;
  const uint64_t tile = tile0 + (SPLIT ? item / groups : item);
  const uint32_t g = SPLIT ? (uint32_t)(item % groups) : 0u;
  const uint64_t row = tile * kWave + lane;
  const bool valid = row < a.nrow;
  float* __restrict__ ta = lds + lane;                       // row tile (exact) / totals (approximate)
  float* __restrict__ ct = lds + (size_t)F * kWave + lane;   // this tree's contributions
  const uint32_t t0 = a.tree_begin + g * trees_per_group;
  const uint32_t t1 = SPLIT ? min(t0 + trees_per_group, a.tree_end) : a.tree_end;
  const uint32_t ntree = a.tree_end - a.tree_begin;
  const bool missing_is_nan = a.missing != a.missing;
  const float* __restrict__ x = a.rows + (valid ? row : 0) * (uint64_t)a.ncol;
  bool any_inf = false;
  if (!APPROX) {
    const float qnan = __builtin_nanf("");
    for (uint32_t f = 0; f < F; ++f) {
      float v = 0.0f;
      if (valid) {
        v = f < a.ncol ? x[f] : qnan;      // columns the matrix does not have are missing
        any_inf |= is_inf(v);
        if (!missing_is_nan && v == a.missing) v = qnan;
      }
      ta[f * kWave] = v;
    }
  } else {
    if (!SPLIT)
      for (uint32_t f = 0; f < F; ++f) ta[f * kWave] = 0.0f;
    // +-inf anywhere in the row, as the exact row tile's fill and predict check - not only where the row's paths
    // split; in the split form the first tree group of each tile looks
    if (valid && a.flags && !is_inf(a.missing) && (!SPLIT || g == 0u))
      for (uint32_t f = 0; f < a.ncol; ++f) any_inf |= is_inf(x[f]);
  }
  float* __restrict__ orow = out + (valid ? row : 0) * (uint64_t)(F + 1);
  for (uint32_t t = t0; t < t1; ++t) {
    for (uint32_t f = 0; f < F; ++f) ct[f * kWave] = 0.0f;
    if (APPROX) {
      if (valid) approx_tree<1>(a, t, x, a.ncol, missing_is_nan, ct);
    } else {
      exact_tree(heads, elems, class_start, coef, t, ta, ct);
    }
    if (SPLIT) {
      float* __restrict__ dst = part + ((tile * ntree + (t - a.tree_begin)) * F) * kWave + lane;
      for (uint32_t f = 0; f < F; ++f) dst[(size_t)f * kWave] = ct[f * kWave];
    } else if (APPROX) {
      for (uint32_t f = 0; f < F; ++f) ta[f * kWave] += ct[f * kWave];
    } else if (valid) {
      for (uint32_t f = 0; f < F; ++f) orow[f] = (t == t0 ? 0.0f : orow[f]) + ct[f * kWave];
    }
  }
  if (!SPLIT && valid) {
    if (APPROX) {
      for (uint32_t f = 0; f < F; ++f) orow[f] = ta[f * kWave];
    } else if (t0 == t1) {
      for (uint32_t f = 0; f < F; ++f) orow[f] = 0.0f;
    }
    orow[F] = a.bias;
  }
  if (any_inf && a.flags && !is_inf(a.missing)) atomicOr(a.flags, 1u);
}

// The second launch of a split: one wave per tile, out[row][f] = ((0 + part[t0][f]) + part[t0 + 1][f]) + ...
__global__ __launch_bounds__(kWave) void contribs_combine_kernel(ContribsArgs a, const float* __restrict__ part) {
  const uint32_t lane = threadIdx.x;
  const uint32_t F = a.nfeat;
  const uint64_t tile = blockIdx.x;
  const uint64_t row = tile * kWave + lane;
  if (row >= a.nrow) return;
  const uint32_t ntree = a.tree_end - a.tree_begin;
  float* __restrict__ orow = a.out + row * (uint64_t)(F + 1);
  const float* __restrict__ src = part + tile * ntree * F * kWave + lane;
  for (uint32_t f = 0; f < F; ++f) {
    float acc = 0.0f;
    for (uint32_t t = 0; t < ntree; ++t) acc += src[((size_t)t * F + f) * kWave];
    orow[f] = acc;
  }
  orow[F] = a.bias;
}

// ---- the fields form (OHXBoosterPredictContribsFields) ----
//
// A tile is 64 consecutive gridcells m of the slab, so each field's load is coalesced.  The gather is the fields
// predict's (kernels.hip fill_tile_fields, restated here so that translation unit stays as tuned): 3-D fields at
// src_off + m, 2-D ones at m % (im * jm), PL / 100 as a float32 division, +-inf noted after it, `missing` -> NaN,
// fields past nfield NaN, a lane without a gridcell 0.  The row tile then feeds the same per-tree arithmetic as the
// rows form (exact_tree, approx_tree), and each tree's vector is added into the totals in tree order from 0.0f, so a
// gridcell's bits are those of its gathered row in OHXBoosterPredictContribs.
// LDS: direct, three [nfeat][64] float tiles (row, tree, totals); split, two (row, tree).  Stores are feature-major:
// per feature 64 consecutive floats of out[f]; a null out[f] is skipped (wave-uniform).
template <bool APPROX, bool SPLIT>
__global__ __launch_bounds__(kWave) void contribs_fields_kernel(ContribsArgs a, FieldsContribsArgs fa, uint64_t tile0,
                                                                uint32_t trees_per_group, uint32_t groups,
                                                                const PathHead* __restrict__ heads,
                                                                const PathElem* __restrict__ elems,
                                                                const uint32_t* __restrict__ class_start,
                                                                const float4* __restrict__ coef,
                                                                float* __restrict__ part) {
  extern __shared__ float lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t F = a.nfeat;
  const uint64_t item = blockIdx.x;
  const uint64_t tile = tile0 + (SPLIT ? item / groups : item);
  const uint32_t g = SPLIT ? (uint32_t)(item % groups) : 0u;
  const uint64_t m = tile * kWave + lane;
  const bool valid = m < fa.nrow;
  float* __restrict__ xt = lds + lane;                            // row tile
  float* __restrict__ ct = lds + (size_t)F * kWave + lane;        // this tree's contributions
  float* __restrict__ tot = lds + (size_t)2 * F * kWave + lane;   // totals (direct)
  const uint32_t t0 = a.tree_begin + g * trees_per_group;
  const uint32_t t1 = SPLIT ? min(t0 + trees_per_group, a.tree_end) : a.tree_end;
  const uint32_t ntree = a.tree_end - a.tree_begin;
  const bool missing_is_nan = fa.missing != fa.missing;
  const float qnan = __builtin_nanf("");
  const uint64_t at3 = fa.src_off + (valid ? m : 0);
  const uint64_t at2 = valid ? m % fa.plane : 0;
  bool any_inf = false;
  for (uint32_t f = 0; f < F; ++f) {
    float v = 0.0f;
    if (valid) {
      v = qnan;
      if (f < fa.nfield) {
        const float* src = fa.field[f];
        v = ((fa.is2d_mask >> f) & 1u) ? src[at2] : src[at3];
        if (f == fa.pl_feature) v = v / 100.0f;
        any_inf |= is_inf(v);
        if (!missing_is_nan && v == fa.missing) v = qnan;
      }
    }
    xt[f * kWave] = v;
  }
  if (!SPLIT)
    for (uint32_t f = 0; f < F; ++f) tot[f * kWave] = 0.0f;
  for (uint32_t t = t0; t < t1; ++t) {
    for (uint32_t f = 0; f < F; ++f) ct[f * kWave] = 0.0f;
    if (APPROX) {
      if (valid) approx_tree<kWave>(a, t, xt, F, true, ct);
    } else {
      exact_tree(heads, elems, class_start, coef, t, xt, ct);
    }
    if (SPLIT) {
      float* __restrict__ dst = part + ((tile * ntree + (t - a.tree_begin)) * F) * kWave + lane;
      for (uint32_t f = 0; f < F; ++f) dst[(size_t)f * kWave] = ct[f * kWave];
    } else {
      for (uint32_t f = 0; f < F; ++f) tot[f * kWave] += ct[f * kWave];
    }
  }
  if (!SPLIT && valid) {
    const uint64_t at = fa.out_off + m;
    for (uint32_t f = 0; f < F; ++f)
      if (fa.out[f] != nullptr) fa.out[f][at] = tot[f * kWave];
    if (fa.out[F] != nullptr) fa.out[F][at] = a.bias;
  }
  if (any_inf && fa.flags && !is_inf(fa.missing)) atomicOr(fa.flags, 1u);
}

// The second launch of a split, as contribs_combine_kernel but feature-major: one wave per tile,
// out[f][out_off + m] = ((0 + part[t0][f]) + part[t0 + 1][f]) + ...
__global__ __launch_bounds__(kWave) void contribs_fields_combine_kernel(ContribsArgs a, FieldsContribsArgs fa,
                                                                        const float* __restrict__ part) {
  const uint32_t lane = threadIdx.x;
  const uint32_t F = a.nfeat;
  const uint64_t tile = blockIdx.x;
  const uint64_t m = tile * kWave + lane;
  if (m >= fa.nrow) return;
  const uint32_t ntree = a.tree_end - a.tree_begin;
  const float* __restrict__ src = part + tile * ntree * F * kWave + lane;
  const uint64_t at = fa.out_off + m;
  for (uint32_t f = 0; f < F; ++f) {
    if (fa.out[f] == nullptr) continue;
    float acc = 0.0f;
    for (uint32_t t = 0; t < ntree; ++t) acc += src[((size_t)t * F + f) * kWave];
    fa.out[f][at] = acc;
  }
  if (fa.out[F] != nullptr) fa.out[F][at] = a.bias;
}

template <bool APPROX>
hipError_t launch_fields_mode(const ContribsArgs& a, const FieldsContribsArgs& fa, const ContribsPlan& plan,
                              float* part, hipStream_t stream) {
  const uint64_t tiles = (fa.nrow + kWave - 1) / kWave;
  const float4* coef = reinterpret_cast<const float4*>(a.coef);
  if (plan.split) {
    const size_t lds = (size_t)2 * a.nfeat * kWave * sizeof(float);
    const uint64_t items = tiles * plan.groups;
    hipLaunchKernelGGL((contribs_fields_kernel<APPROX, true>), dim3((unsigned)items), dim3(kWave), lds, stream, a, fa,
                       (uint64_t)0, plan.trees_per_group, plan.groups, a.heads, a.elems, a.class_start, coef, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(contribs_fields_combine_kernel, dim3((unsigned)tiles), dim3(kWave), 0, stream, a, fa,
                       (const float*)part);
    return hipGetLastError();
  }
  const size_t lds = (size_t)3 * a.nfeat * kWave * sizeof(float);
  const uint64_t chunk = APPROX ? (1ull << 24) : kDirectTilesPerLaunch;
  for (uint64_t t = 0; t < tiles; t += chunk) {
    const uint64_t n = tiles - t < chunk ? tiles - t : chunk;
    hipLaunchKernelGGL((contribs_fields_kernel<APPROX, false>), dim3((unsigned)n), dim3(kWave), lds, stream, a, fa, t,
                       0u, 1u, a.heads, a.elems, a.class_start, coef, (float*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <bool APPROX>
hipError_t launch_mode(const ContribsArgs& a, const ContribsPlan& plan, float* part, hipStream_t stream) {
  const uint64_t tiles = (a.nrow + kWave - 1) / kWave;
  const size_t lds = (size_t)2 * a.nfeat * kWave * sizeof(float);
  const float4* coef = reinterpret_cast<const float4*>(a.coef);
  if (plan.split) {
    const uint64_t items = tiles * plan.groups;
    hipLaunchKernelGGL((contribs_kernel<APPROX, true>), dim3((unsigned)items), dim3(kWave), lds, stream, a, (uint64_t)0,
                       plan.trees_per_group, plan.groups, a.heads, a.elems, a.class_start, coef, a.out, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(contribs_combine_kernel, dim3((unsigned)tiles), dim3(kWave), 0, stream, a, (const float*)part);
    return hipGetLastError();
  }
  const uint64_t chunk = APPROX ? (1ull << 24) : kDirectTilesPerLaunch;
  for (uint64_t t = 0; t < tiles; t += chunk) {
    const uint64_t n = tiles - t < chunk ? tiles - t : chunk;
    hipLaunchKernelGGL((contribs_kernel<APPROX, false>), dim3((unsigned)n), dim3(kWave), lds, stream, a, t, 0u, 1u,
                       a.heads, a.elems, a.class_start, coef, a.out, (float*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

int launch_contribs(bool approximate, const ContribsArgs& a, const ContribsPlan& plan, float* part, void* stream) {
  if (a.nrow == 0) return (int)hipSuccess;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return (int)(approximate ? launch_mode<true>(a, plan, part, s) : launch_mode<false>(a, plan, part, s));
}

int launch_contribs_fields(bool approximate, const ContribsArgs& a, const FieldsContribsArgs& f,
                           const ContribsPlan& plan, float* part, void* stream) {
  if (f.nrow == 0) return (int)hipSuccess;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return (int)(approximate ? launch_fields_mode<true>(a, f, plan, part, s)
                           : launch_fields_mode<false>(a, f, plan, part, s));
}

}  // namespace ohx
