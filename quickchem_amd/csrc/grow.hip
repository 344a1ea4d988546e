// gfx950 kernels of the tree grower (grow.hpp; design in docs/18_boost_trees.md).
//
//   grow_bin_kernel        once per call: the cuts are staged in LDS, a lane takes a row and finds each value's bin by
//                          binary search; bins[f][row] is feature-major, so a wave's 64 bins are 64 contiguous bytes.
//   grow_hist_kernel       once per level: a lane takes a row, recomputes q from pred and the label, and adds it into
//                          the block's LDS histogram of its (node group, feature group) with a 64-bit integer add, the
//                          row count with a 32-bit one; the block flushes its nonzero bins once with 64-bit global adds.
//   grow_split_kernel<0>   once per level: a wave per (node, feature) - integer prefix sums across the 256 bins, the
//                          shared gain in double, and a butterfly reduction by the total order of grow_better.
//   grow_split_kernel<1>   once per level, one block: a thread per open node takes the best of its features, the
//                          splitting nodes get their child ids in ascending node order, the records are written.
//   grow_partition_kernel  once per level: a row on a node that split steps to the child its bin says.
//   grow_leaf_kernel       once per tree: pred += leaf[pos], pos = 0.
// Only integer adds: no float atomics, no compare-and-swap loops, and the same trees whatever the order of the rows or
// the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grow.hpp"
#include "walk_device.hpp"

namespace ohx {

namespace {

constexpr int kBlock = (int)kGrowBlock;
constexpr int kHistBlock = (int)kGrowHistBlock;

// the open nodes of level `level`: the root alone at level 0, whatever the state word still holds from the last tree
__device__ inline void level_range(const GrowArgs& a, uint32_t level, uint32_t* begin, uint32_t* end, uint32_t* next) {
  if (level == 0) {
    *begin = 0;
    *end = 1;
    *next = 1;
  } else {
    *begin = a.state->begin;
    *end = a.state->end;
    *next = a.state->next;
  }
}

// grid (blocks); dynamic LDS: the cuts
__global__ __launch_bounds__(kBlock) void grow_bin_kernel(GrowArgs a) {
  extern __shared__ float grow_cuts[];
  for (uint32_t i = threadIdx.x; i < a.ncuts; i += kBlock) grow_cuts[i] = a.cuts[i];
  __syncthreads();
  const bool missing_is_nan = a.missing != a.missing;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const float* x = a.rows + row * (uint64_t)a.ncol;
    for (uint32_t f = 0; f < a.num_feature; ++f) {
      const uint32_t c0 = a.cut_ptr[f], c1 = a.cut_ptr[f + 1];
      uint32_t b = kGrowMissingBin;
      if (f < a.ncol) {
        const float v = x[f];
        if (!(v != v || (!missing_is_nan && v == a.missing))) {
          // b = #{j : c_j <= v}
          uint32_t lo = c0, hi = c1;
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (grow_cuts[mid] <= v) lo = mid + 1;
            else hi = mid;
          }
          b = lo - c0;
        }
      }
      a.bins[(uint64_t)f * a.nrow + row] = (uint8_t)b;
    }
  }
}

// grid (blocks over the rows, node groups x feature groups); dynamic LDS: node_group x feat_group x 256 x (8 + 4)
__global__ __launch_bounds__(kHistBlock) void grow_hist_kernel(GrowArgs a, uint32_t level, uint32_t node_group,
                                                               uint32_t feat_group, uint32_t feat_groups) {
  extern __shared__ unsigned long long grow_hist[];
  uint32_t begin, end, next;
  level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  const uint32_t slot0 = (blockIdx.y / feat_groups) * node_group;
  const uint32_t f0 = (blockIdx.y % feat_groups) * feat_group;
  if (slot0 >= count || f0 >= a.num_feature) return;
  const uint32_t nslots = count - slot0 < node_group ? count - slot0 : node_group;
  const uint32_t nf = a.num_feature - f0 < feat_group ? a.num_feature - f0 : feat_group;
  const uint32_t cells = node_group * feat_group * kGrowBins;
  unsigned long long* Gl = grow_hist;
  uint32_t* Hl = reinterpret_cast<uint32_t*>(grow_hist + cells);
  for (uint32_t i = threadIdx.x; i < cells; i += kHistBlock) {
    Gl[i] = 0ull;
    Hl[i] = 0u;
  }
  __syncthreads();
  const uint32_t first = begin + slot0;
  const uint64_t stride = (uint64_t)gridDim.x * kHistBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kHistBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t s = (uint32_t)a.pos[row] - first;   // (a node below `first` wraps past nslots)
    if (s >= nslots) continue;
    const float g = a.pred[row] - a.labels[row];
    // (a NaN fails the comparison)
    if (!(__builtin_fabsf(g) < kRefitMaxAbsGrad)) {
      atomicOr(&a.state->error, kGrowFlagLabel);
      continue;
    }
    const unsigned long long q = (unsigned long long)(long long)__builtin_rintf(g * kRefitGradScale);
    const uint8_t* bin = a.bins + (uint64_t)f0 * a.nrow + row;
    const uint32_t base = s * feat_group * kGrowBins;
    for (uint32_t k = 0; k < nf; ++k) {
      const uint32_t i = base + k * kGrowBins + bin[(uint64_t)k * a.nrow];
      atomicAdd(&Gl[i], q);
      atomicAdd(&Hl[i], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < cells; i += kHistBlock) {
    const uint32_t h = Hl[i];
    if (h == 0u) continue;
    const uint32_t s = i / (feat_group * kGrowBins), k = (i / kGrowBins) % feat_group, b = i % kGrowBins;
    if (s >= nslots || k >= nf) continue;
    const uint64_t gi = ((uint64_t)(slot0 + s) * a.num_feature + f0 + k) * kGrowBins + b;
    atomicAdd(&a.Hhist[gi], (unsigned long long)h);
    const unsigned long long g = Gl[i];
    if (g != 0ull) atomicAdd(&a.Ghist[gi], g);
  }
}

__device__ inline GrowCand shuffle_cand(const GrowCand& c, int d) {
  GrowCand o;
  o.loss_chg = __shfl_xor(c.loss_chg, d, kWave);
  o.GL = __shfl_xor((long long)c.GL, d, kWave);
  o.HL = __shfl_xor((unsigned long long)c.HL, d, kWave);
  o.key = __shfl_xor(c.key, d, kWave);
  o.valid = __shfl_xor(c.valid, d, kWave);
  return o;
}

__device__ inline void write_leaf(const GrowArgs& a, GrowNode* nodes, uint32_t n, int64_t G, uint64_t H, int32_t parent) {
  float leaf, weight;
  refit_solve_leaf(G, H, a.eta, a.lambda, &leaf, &weight);
  GrowNode r;
  r.G = G;
  r.H = H;
  r.left = r.right = -1;
  r.parent = parent;
  r.feature = r.cut = r.default_left = 0;
  r.value = leaf;
  r.loss_chg = 0.0f;
  r.sum_hess = (float)H;
  r.base_weight = weight;
  nodes[n] = r;
}

// PHASE 0: grid (blocks of four waves over slots x features).  PHASE 1: one block.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void grow_split_kernel(GrowArgs a, uint32_t level, uint32_t round) {
  uint32_t begin, end, next;
  level_range(a, level, &begin, &end, &next);
  const uint32_t count = end - begin;
  const uint32_t F = a.num_feature;
  GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  if (PHASE == 0) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t w = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    const uint32_t slot = w / F, f = w % F;
    if (slot >= count) return;
    const uint64_t at = ((uint64_t)slot * F + f) * kGrowBins + 4u * lane;
    int64_t g4[4];
    uint64_t h4[4];
    int64_t gs = 0;
    uint64_t hs = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      g4[k] = (int64_t)a.Ghist[at + k];
      h4[k] = (uint64_t)a.Hhist[at + k];
      gs += g4[k];
      hs += h4[k];
    }
    // inclusive sums across the wave, then the sums below the lane's first bin
    long long gi = gs;
    unsigned long long hi = hs;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const long long gt = __shfl_up(gi, d, kWave);
      const unsigned long long ht = __shfl_up(hi, d, kWave);
      if (lane >= d) {
        gi += gt;
        hi += ht;
      }
    }
    const int64_t Gp = __shfl(gi, kWave - 1, kWave);
    const uint64_t Hp = __shfl(hi, kWave - 1, kWave);
    const int64_t Gm = __shfl((long long)g4[3], kWave - 1, kWave);
    const uint64_t Hm = __shfl((unsigned long long)h4[3], kWave - 1, kWave);
    if (level == 0 && f == 0 && lane == 0) {   // the root's sums: every row is in one bin of feature 0
      nodes[0].G = Gp;
      nodes[0].H = Hp;
    }
    const uint32_t ncut = a.cut_ptr[f + 1] - a.cut_ptr[f];
    GrowCand c = grow_best_split(g4, h4, f, 4u * lane, 4u, ncut, gi - gs, hi - hs, Gm, Hm, Gp, Hp, (double)a.lambda,
                                 a.min_child_rows);
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const GrowCand o = shuffle_cand(c, d);
      if (grow_better(o, c)) c = o;
    }
    if (lane == 0) a.best[(uint64_t)slot * F + f] = c;
  } else {
    __shared__ uint32_t splits[kGrowMaxNodes / 2];
    const uint32_t s = threadIdx.x;
    const bool active = s < count && s < kGrowMaxNodes / 2;
    const uint32_t node = begin + s;
    GrowCand best;
    int64_t Gp = 0;
    uint64_t Hp = 0;
    if (active) {
      Gp = nodes[node].G;
      Hp = nodes[node].H;
      if (level == 0) write_leaf(a, nodes, 0, Gp, Hp, -1);
      for (uint32_t f = 0; f < F; ++f) {
        const GrowCand c = a.best[(uint64_t)s * F + f];
        if (grow_better(c, best)) best = c;
      }
    }
    const bool split = active && best.valid && best.loss_chg > (double)a.gamma;
    if (s < kGrowMaxNodes / 2) splits[s] = split ? 1u : 0u;
    __syncthreads();
    uint32_t below = 0, total = 0;
    const uint32_t live = count < kGrowMaxNodes / 2 ? count : kGrowMaxNodes / 2;
    for (uint32_t i = 0; i < live; ++i) {
      total += splits[i];
      if (i < s) below += splits[i];
    }
    if (next + 2u * total > kGrowMaxNodes) {   // (never: a tree of depth 8 has 511 nodes)
      if (s == 0) atomicOr(&a.state->error, kGrowFlagState);
      total = 0;
    } else if (split) {
      const uint32_t f = best.key >> 9, j = (best.key >> 1) & 255u, dl = best.key & 1u;
      const uint32_t left = next + 2u * below;
      nodes[node].left = (int32_t)left;
      nodes[node].right = (int32_t)left + 1;
      nodes[node].feature = f;
      nodes[node].cut = j;
      nodes[node].default_left = dl;
      nodes[node].value = a.cuts[a.cut_ptr[f] + j];
      nodes[node].loss_chg = (float)best.loss_chg;
      write_leaf(a, nodes, left, best.GL, best.HL, (int32_t)(node | 0x80000000u));
      write_leaf(a, nodes, left + 1, Gp - best.GL, Hp - best.HL, (int32_t)node);
    }
    if (s == 0) {
      a.state->begin = next;
      a.state->end = next + 2u * total;
      a.state->next = next + 2u * total;
      a.tree_nodes[round] = next + 2u * total;
    }
  }
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_partition_kernel(GrowArgs a, uint32_t round) {
  const GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const uint32_t next = a.state->next;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t p = a.pos[row];
    if (p >= next) {
      atomicOr(&a.state->error, kGrowFlagState);
      continue;
    }
    const int32_t left = nodes[p].left;
    if (left < 0) continue;
    const uint32_t f = nodes[p].feature;
    if (f >= a.num_feature) {
      atomicOr(&a.state->error, kGrowFlagState);
      continue;
    }
    const uint32_t b = a.bins[(uint64_t)f * a.nrow + row];
    const bool go_left = b == kGrowMissingBin ? nodes[p].default_left != 0u : b <= nodes[p].cut;
    a.pos[row] = (uint16_t)(go_left ? left : nodes[p].right);
  }
}

// grid (blocks)
__global__ __launch_bounds__(kBlock) void grow_leaf_kernel(GrowArgs a, uint32_t round) {
  const GrowNode* nodes = a.nodes + (uint64_t)round * kGrowMaxNodes;
  const uint32_t next = a.state->next;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x; row < a.nrow; row += stride) {
    const uint32_t p = a.pos[row];
    if (p < next) a.pred[row] += nodes[p].value;
    else atomicOr(&a.state->error, kGrowFlagState);
    a.pos[row] = 0;
  }
}

}  // namespace

int prepare_grow() {
  hipError_t e = raise_lds_limit(grow_bin_kernel, kGrowMaxFeatures * kGrowMaxCuts * sizeof(float));
  if (e != hipSuccess) return e;
  return raise_lds_limit(grow_hist_kernel, kGrowMaxPairs * kGrowPairBytes);
}

int launch_grow_bin(const GrowArgs& a, const GrowPlan& plan, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || a.ncol > a.num_feature || a.num_feature == 0 ||
      a.num_feature > kGrowMaxFeatures || (uint64_t)a.ncuts > (uint64_t)a.num_feature * kGrowMaxCuts ||
      plan.bin_lds_bytes != a.ncuts * sizeof(float) || plan.row_blocks == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_bin_kernel, dim3(plan.row_blocks), dim3(kBlock), plan.bin_lds_bytes, stream, a);
  return hipGetLastError();
}

int launch_grow_tree(const GrowArgs& a, const GrowPlan& plan, uint32_t round, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || a.max_depth < 1 ||
      a.max_depth > kGrowMaxDepth || plan.levels.size() != (size_t)a.max_depth || plan.row_blocks == 0 || a.min_child_rows < 1)
    return hipErrorInvalidValue;
  const uint32_t F = a.num_feature;
  hipError_t e = hipSuccess;
  for (uint32_t d = 0; d < (uint32_t)a.max_depth; ++d) {
    const GrowLevelPlan& l = plan.levels[d];
    if (l.slots != (1u << d) || l.node_group * l.feat_group > kGrowMaxPairs || l.node_group == 0 || l.feat_group == 0 ||
        l.lds_bytes != l.node_group * l.feat_group * kGrowPairBytes || l.node_groups * l.node_group < l.slots ||
        l.feat_groups * l.feat_group < F || l.hist_blocks == 0 ||
        (a.nrow + (uint64_t)l.hist_blocks * kGrowHistBlock - 1) / ((uint64_t)l.hist_blocks * kGrowHistBlock) > kGrowMaxTrips)
      return hipErrorInvalidValue;
    const size_t bytes = (size_t)l.slots * F * kGrowBins * sizeof(unsigned long long);
    if ((e = hipMemsetAsync(a.Ghist, 0, bytes, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.Hhist, 0, bytes, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(grow_hist_kernel, dim3(l.hist_blocks, l.node_groups * l.feat_groups), dim3(kHistBlock), l.lds_bytes,
                       stream, a, d, l.node_group, l.feat_group, l.feat_groups);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t waves = l.slots * F, per_block = kBlock / kWave;
    hipLaunchKernelGGL(grow_split_kernel<0>, dim3((waves + per_block - 1) / per_block), dim3(kBlock), 0, stream, a, d, round);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(grow_split_kernel<1>, dim3(1), dim3(kBlock), 0, stream, a, d, round);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(grow_partition_kernel, dim3(plan.row_blocks), dim3(kBlock), 0, stream, a, round);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(grow_leaf_kernel, dim3(plan.row_blocks), dim3(kBlock), 0, stream, a, round);
  return hipGetLastError();
}

int launch_grow_partition(const GrowArgs& a, const GrowPlan& plan, uint32_t round, void* stream_) {
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || a.num_feature == 0 || a.num_feature > kGrowMaxFeatures || plan.row_blocks == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_partition_kernel, dim3(plan.row_blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream_), a, round);
  return hipGetLastError();
}

int launch_grow_leaf(const GrowArgs& a, const GrowPlan& plan, uint32_t round, void* stream_) {
  if (a.nrow == 0 || a.nrow > kRefitMaxRows || plan.row_blocks == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grow_leaf_kernel, dim3(plan.row_blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream_), a, round);
  return hipGetLastError();
}

}  // namespace ohx
