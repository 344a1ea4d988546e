// libohx_synth.so — host-only generator of the synthetic benchmark inputs of
// the 27-feature batches (same definition as the device
// generator, synth_common.h) and the synthetic OH booster (T trees of depth <= D
// grown by recursive partitioning of a feature sample, thresholds taken from the
// sample itself so that x == threshold ties occur).
//
// The reference ships no model file and no data (its production models live on
// NCCS paths, OH_GridComp/OH_instance_OH.rc:17-20), so every test and benchmark
// input comes from here.  Nothing in this file predicts anything.
#include <algorithm>
#include <cmath>
#ifdef _OPENMP
#include <omp.h>
#endif
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "cells.hpp"
#include "flatten.hpp"
#include "forest.hpp"
#include "super_walk.hpp"
#include "synth_common.h"

using namespace ohx;

namespace {

thread_local std::string g_err;

struct Work {
  int32_t node;
  uint32_t lo, hi;
  int depth;
};

inline void cell_of(uint64_t m, int im, int jm, int* i, int* j, int* k) {
  const uint64_t plane = (uint64_t)im * (uint64_t)jm;
  *k = (int)(m / plane);
  const uint64_t c = m - (uint64_t)(*k) * plane;
  *j = (int)(c / (uint64_t)im);
  *i = (int)(c - (uint64_t)(*j) * (uint64_t)im);
}

}  // namespace

namespace ohx {
void synth_set_error(const std::string& m) { g_err = m; }   // for contribs_host.cpp
}

#pragma GCC visibility push(default)
extern "C" {

const char* ohx_synth_last_error(void) { return g_err.c_str(); }

// torch.distributed.run exports OMP_NUM_THREADS=1 to every rank; the generators are told their
// share of the host cores explicitly instead.
void ohx_synth_set_threads(int n) {
#ifdef _OPENMP
  if (n > 0) omp_set_num_threads(n);
#else
  (void)n;
#endif
}

// rows [nrows][27], PL in hPa (as xx_carr holds it, OH_GridCompMod.F90:314)
int ohx_synth_rows_cpu(uint32_t seed, int im, int jm, int km, uint64_t row_begin, uint64_t nrows, float* out) {
  if (im <= 0 || jm <= 0 || km <= 0 || row_begin + nrows > (uint64_t)im * jm * km) {
    g_err = "ohx_synth_rows_cpu: bad grid or row range";
    return -1;
  }
#pragma omp parallel for schedule(static)
  for (int64_t r = 0; r < (int64_t)nrows; ++r) {
    int i, j, k;
    cell_of(row_begin + (uint64_t)r, im, jm, &i, &j, &k);
    for (int f = 0; f < OHX_NFEAT; ++f) out[(uint64_t)r * OHX_NFEAT + f] = ohx_synth_feature(seed, f, i, j, k, im, jm, km);
  }
  return 0;
}

// one MAPL field: feature 0..26 ((im,jm) for the 2-D ones, else (im,jm,km); PL in Pa), -1 = TROPP in Pa
int ohx_synth_field_cpu(uint32_t seed, int feature, int im, int jm, int km, float* out) {
  if (im <= 0 || jm <= 0 || km <= 0 || feature < -1 || feature >= OHX_NFEAT) {
    g_err = "ohx_synth_field_cpu: bad argument";
    return -1;
  }
  const bool two_d = feature < 0 || ohx_feature_is_2d(feature);
  const int64_t total = (int64_t)im * jm * (two_d ? 1 : km);
#pragma omp parallel for schedule(static)
  for (int64_t m = 0; m < total; ++m) {
    int i, j, k;
    cell_of((uint64_t)m, im, jm, &i, &j, &k);
    float v;
    if (feature < 0) v = ohx_synth_tropp_pa(seed, i, j);
    else if (feature == OHX_F_PL) v = ohx_synth_pl_pa(seed, i, j, k, im, jm, km);
    else v = ohx_synth_feature(seed, feature, i, j, k, im, jm, km);
    out[m] = v;
  }
  return 0;
}

// Grow the synthetic booster and return it as a model file image (malloc'd):
// format 0 = XGBoost legacy binary, 1 = JSON.  The feature sample is 2**sample_log2
// cells of the (im,jm,km) grid generated with feature_seed.
//   stats[0] = total nodes, stats[1] = total leaves, stats[2] = max depth,
//   stats[3] = sum over sample rows and trees of the walk length (internal nodes visited)
int ohx_synth_model(uint32_t model_seed, int num_trees, int max_depth, int sample_log2, int min_leaf,
                    uint32_t feature_seed, int im, int jm, int km, float base_score, float leaf_sigma, int format,
                    uint8_t** out_buf, uint64_t* out_len, uint64_t stats[4]) {
  try {
    if (num_trees < 0 || max_depth < 0 || max_depth > 40 || sample_log2 < 1 || sample_log2 > 26 || min_leaf < 1 ||
        im <= 0 || jm <= 0 || km <= 0 || out_buf == nullptr || out_len == nullptr)
      throw OhxError("ohx_synth_model: bad argument");
    const uint32_t S = 1u << sample_log2;
    const uint64_t ncell = (uint64_t)im * jm * km;
    // feature-major sample: X[f][s]
    std::vector<float> X((size_t)OHX_NFEAT * S);
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < (int64_t)S; ++s) {
      const uint32_t h1 = ohx_hash4(model_seed, 0xA1u, (uint32_t)s, 0u, 0u);
      const uint32_t h2 = ohx_hash4(model_seed, 0xA2u, (uint32_t)s, 0u, 0u);
      const uint64_t m = (((uint64_t)h1 << 32) | h2) % ncell;
      int i, j, k;
      cell_of(m, im, jm, &i, &j, &k);
      for (int f = 0; f < OHX_NFEAT; ++f) X[(size_t)f * S + (size_t)s] = ohx_synth_feature(feature_seed, f, i, j, k, im, jm, km);
    }
    Forest forest;
    forest.base_score = base_score;
    forest.num_feature = OHX_NFEAT;
    forest.objective = "reg:squarederror";
    forest.trees.resize((size_t)num_trees);
    forest.tree_info.assign((size_t)num_trees, 0);
    std::vector<uint64_t> walk_sum((size_t)num_trees, 0), leaves((size_t)num_trees, 0);
    std::vector<int> depth_max((size_t)num_trees, 0);
#pragma omp parallel for schedule(dynamic, 1)
    for (int t = 0; t < num_trees; ++t) {
      std::vector<uint32_t> idx(S);
      for (uint32_t s = 0; s < S; ++s) idx[s] = s;
      std::vector<int32_t> left, right, parent;
      std::vector<uint32_t> feat;
      std::vector<uint8_t> dl;
      std::vector<float> value, hess;
      auto new_node = [&](int32_t par) {
        left.push_back(-1);
        right.push_back(-1);
        parent.push_back(par);
        feat.push_back(0);
        dl.push_back(0);
        value.push_back(0.0f);
        hess.push_back(0.0f);
        return (int32_t)left.size() - 1;
      };
      std::deque<Work> queue;
      queue.push_back({new_node(-1), 0u, S, 0});
      while (!queue.empty()) {
        const Work w = queue.front();
        queue.pop_front();
        const uint32_t cnt = w.hi - w.lo;
        hess[(size_t)w.node] = (float)cnt;
        bool split = false;
        if (w.depth < max_depth && cnt >= 2u * (uint32_t)min_leaf) {
          for (uint32_t attempt = 0; attempt < 8 && !split; ++attempt) {
            const uint32_t h = ohx_hash4(model_seed, 0xB0u + attempt, (uint32_t)t, (uint32_t)w.node, 0u);
            const uint32_t f = h % OHX_NFEAT;
            const uint32_t pick = w.lo + ohx_hash4(model_seed, 0xC0u + attempt, (uint32_t)t, (uint32_t)w.node, 1u) % cnt;
            const float* xf = &X[(size_t)f * S];
            const float thr = xf[idx[pick]];
            uint32_t* b = idx.data() + w.lo;
            uint32_t* e = idx.data() + w.hi;
            uint32_t* mid = std::partition(b, e, [&](uint32_t s) { return xf[s] < thr; });
            const uint32_t nl = (uint32_t)(mid - b);
            if (nl >= (uint32_t)min_leaf && cnt - nl >= (uint32_t)min_leaf) {
              const int32_t l = new_node((int32_t)((uint32_t)w.node | 0x80000000u));
              const int32_t r = new_node(w.node);
              left[(size_t)w.node] = l;
              right[(size_t)w.node] = r;
              feat[(size_t)w.node] = f;
              dl[(size_t)w.node] = (uint8_t)((h >> 16) & 1u);
              value[(size_t)w.node] = thr;
              queue.push_back({l, w.lo, w.lo + nl, w.depth + 1});
              queue.push_back({r, w.lo + nl, w.hi, w.depth + 1});
              split = true;
            }
          }
        }
        if (!split) {
          const uint32_t a = ohx_hash4(model_seed, 0xD0u, (uint32_t)t, (uint32_t)w.node, 0u);
          const uint32_t c = ohx_hash4(model_seed, 0xD1u, (uint32_t)t, (uint32_t)w.node, 0u);
          // sum of four uniforms: variance 1/3
          const float g = (ohx_u01(a) + ohx_u01(a * 0x9E3779B1u + 1u) + ohx_u01(c) + ohx_u01(c * 0x85EBCA77u + 1u)) - 2.0f;
          value[(size_t)w.node] = g * 1.7320508f * leaf_sigma;
          leaves[(size_t)t] += 1;
          walk_sum[(size_t)t] += (uint64_t)cnt * (uint64_t)w.depth;
          depth_max[(size_t)t] = std::max(depth_max[(size_t)t], w.depth);
        }
      }
      Tree& tr = forest.trees[(size_t)t];
      tr.resize(left.size());
      tr.left = left;
      tr.right = right;
      tr.parent = parent;
      tr.feature = feat;
      tr.default_left = dl;
      tr.value = value;
      tr.sum_hess = hess;
      tr.num_feature = OHX_NFEAT;
    }
    forest.validate();
    if (stats) {
      stats[0] = forest.total_nodes();
      stats[1] = 0;
      stats[2] = 0;
      stats[3] = 0;
      for (int t = 0; t < num_trees; ++t) {
        stats[1] += leaves[(size_t)t];
        stats[2] = std::max<uint64_t>(stats[2], (uint64_t)depth_max[(size_t)t]);
        stats[3] += walk_sum[(size_t)t];
      }
    }
    if (format == 1) {
      std::string s = write_json_model(forest);
      *out_buf = (uint8_t*)malloc(s.size());
      if (*out_buf == nullptr) throw OhxError("ohx_synth_model: out of memory");
      memcpy(*out_buf, s.data(), s.size());
      *out_len = s.size();
    } else {
      std::vector<uint8_t> b = write_legacy_binary(forest);
      *out_buf = (uint8_t*)malloc(b.size());
      if (*out_buf == nullptr) throw OhxError("ohx_synth_model: out of memory");
      memcpy(*out_buf, b.data(), b.size());
      *out_len = b.size();
    }
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

void ohx_synth_free(uint8_t* buf) { free(buf); }

// Convert a model file image between the formats (host logic of XGBoosterLoadModel/SaveModel
// without a booster): 0 = legacy binary, 1 = JSON, 2 = UBJSON.
int ohx_model_convert(const uint8_t* in_buf, uint64_t in_len, int format, uint8_t** out_buf, uint64_t* out_len) {
  try {
    Forest f = load_model_buffer(in_buf, (size_t)in_len);
    f.validate();
    if (format == 1) {
      std::string s = write_json_model(f);
      *out_buf = (uint8_t*)malloc(s.size());
      memcpy(*out_buf, s.data(), s.size());
      *out_len = s.size();
    } else {
      std::vector<uint8_t> b = format == 2 ? write_ubjson_model(f) : write_legacy_binary(f);
      *out_buf = (uint8_t*)malloc(b.size());
      memcpy(*out_buf, b.data(), b.size());
      *out_len = b.size();
    }
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// Host check of the super-node layout (flatten.hpp), for the CPU test-suite: walks emit_super's arrays
// the way the kernels do - the root from the head record (phase 1), a fixed `steps` iterations per tree,
// no finished state, the leaf OR-ed in whenever the child's code is 31, fillers after it - so that a
// layout bug shows without a GPU.  Not a prediction path: scalar, test support only.
// out[nrow] margins; info[0] = super-nodes, info[1] = trees that start below the root (phase 1),
// info[2] = total steps.  Returns 1 if the booster does not fit the format.
int ohx_super_walk_pack_cpu(const uint8_t* model, uint64_t model_len, int super_pack, const float* rows, uint64_t nrow,
                             uint32_t ncol, float missing, float* out, uint64_t* info);
int ohx_super_walk_cpu(const uint8_t* model, uint64_t model_len, const float* rows, uint64_t nrow, uint32_t ncol,
                       float missing, float* out, uint64_t* info) {
  return ohx_super_walk_pack_cpu(model, model_len, LayoutParams().super_pack, rows, nrow, ncol, missing, out, info);
}

// ... with the groups placed as `super_pack` says (flatten.hpp kSuperPack*), the default being what a booster uploads
int ohx_super_walk_pack_cpu(const uint8_t* model, uint64_t model_len, int super_pack, const float* rows, uint64_t nrow,
                             uint32_t ncol, float missing, float* out, uint64_t* info) {
  try {
    Forest f = load_model_buffer(model, (size_t)model_len);
    f.validate();
    SuperForest sf;
    if (!emit_super(f, &sf, super_pack)) return 1;
    uint64_t phase1 = 0, steps = 0;
    for (const SuperTreeHead& h : sf.heads) {
      phase1 += (h.root_meta >> 8) & 1u;
      steps += h.steps;
    }
    if (info) {
      info[0] = sf.nodes.size();
      info[1] = phase1;
      info[2] = steps;
    }
    std::vector<float> x(32, 0.0f);   // rows 27..31 "belong to nobody"
    for (uint64_t r = 0; r < nrow; ++r) {
      super_walk_row(rows + r * ncol, ncol, f.num_feature, missing, x.data());
      float acc = f.base_score;
      // two more steps than the tree has, as when it shares a group of chains with a deeper tree (a walk past its
      // leaf only meets fillers)
      for (const SuperTreeHead& h : sf.heads) acc += super_walk_tree(sf, h, x.data(), h.steps + 2u, nullptr);
      out[r] = acc;
    }
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// emit_super's arrays themselves, for the CPU test-suite's checks of what flatten.hpp promises: nodes = four 32-bit
// words per record {thr0, thrL, thrR as float bits, meta}, heads = four words per tree {base, root_meta, root_thr
// bits, steps}, packed = per tree 1 if its deep groups were numbered by line.  info[0] = records, info[1] = trees;
// every array is written up to its cap (caps 0: ask for the sizes).  Returns 1 if the booster does not fit the format.
int ohx_super_records_cpu(const uint8_t* model, uint64_t model_len, int super_pack, uint32_t* nodes, uint64_t cap_nodes,
                          uint32_t* heads, uint8_t* packed, uint64_t cap_trees, uint64_t* info) {
  try {
    Forest f = load_model_buffer(model, (size_t)model_len);
    f.validate();
    SuperForest sf;
    if (!emit_super(f, &sf, super_pack)) return 1;
    info[0] = sf.nodes.size();
    info[1] = sf.heads.size();
    static_assert(sizeof(SuperNode) == 16 && sizeof(SuperTreeHead) == 16, "four words each");
    if (cap_nodes) memcpy(nodes, sf.nodes.data(), std::min<size_t>(cap_nodes, sf.nodes.size()) * 16);
    if (cap_trees) {
      memcpy(heads, sf.heads.data(), std::min<size_t>(cap_trees, sf.heads.size()) * 16);
      memcpy(packed, sf.packed.data(), std::min<size_t>(cap_trees, sf.packed.size()));
    }
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// Distinct cache lines per deep gather (line_count.cpp count_super_lines, which says what rows and shape mean; shape =
// {li, lj, lk, k_fastest}, NULL or all 0: 64 consecutive rows a wave).  table: six doubles per step for steps 0 ..
// 31 - wave-gathers, then the sums of distinct records, of look-ups, of 128-byte lines, then blocks of 16 tiles and the
// sum of their distinct lines.  info[0] = records of the forest, info[1] = fillers among them, info[2] = trees
// numbered by line.  Returns 1 if the booster does not fit the format.
int ohx_super_line_count(const uint8_t* model, uint64_t model_len, int super_pack, const float* rows, uint64_t ntile,
                         uint32_t ncol, float missing, const uint32_t* shape, uint32_t first_step, double* table,
                         uint64_t* info) {
  try {
    Forest f = load_model_buffer(model, (size_t)model_len);
    f.validate();
    SuperForest sf;
    if (!emit_super(f, &sf, super_pack)) return 1;
    LineCountShape sh;
    if (shape) sh.li = shape[0], sh.lj = shape[1], sh.lk = shape[2], sh.k_fastest = shape[3];
    if (sh.li + sh.lj + sh.lk != 6 && sh.li + sh.lj + sh.lk != 0) throw OhxError("ohx_super_line_count: a brick is 64 gridcells");
    std::vector<LineCountStep> steps(kLineCountMaxSteps);
    count_super_lines(sf, f.num_feature, rows, ntile, ncol, missing, sh, first_step, steps.data());
    for (uint32_t s = 0; s < kLineCountMaxSteps; ++s) {
      const LineCountStep& st = steps[s];
      const double row[6] = {st.gathers, st.records, st.lookups, st.lines, st.block_gathers, st.block_lines};
      memcpy(table + 6 * s, row, sizeof row);
    }
    if (info) {
      uint64_t fillers = 0, by_line = 0;
      const uint32_t filler_meta = super_meta(0, 0, 0, 1, 1, 1, 0);
      for (const SuperNode& n : sf.nodes) fillers += n.meta == filler_meta && std::isinf(n.thr0);
      for (uint8_t p : sf.packed) by_line += p;
      info[0] = sf.nodes.size();
      info[1] = fillers;
      info[2] = by_line;
    }
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// What emit_super made of every tree, for the CPU test-suite (which edge classes a test booster reaches): out[2 t] =
// phase of tree t (1: the root is evaluated from the head record), out[2 t + 1] = its steps.  *ntrees = trees of the
// booster; at most `cap` pairs are written (cap 0: ask for the count).  Returns 1 if the booster does not fit the format.
int ohx_super_heads_cpu(const uint8_t* model, uint64_t model_len, uint32_t* out, uint64_t cap, uint64_t* ntrees) {
  try {
    Forest f = load_model_buffer(model, (size_t)model_len);
    f.validate();
    SuperForest sf;
    if (!emit_super(f, &sf)) return 1;
    *ntrees = sf.heads.size();
    for (size_t t = 0; t < sf.heads.size() && t < cap; ++t) {
      out[2 * t] = (sf.heads[t].root_meta >> 8) & 1u;
      out[2 * t + 1] = sf.heads[t].steps;
    }
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// What emit_cat (flatten.hpp) makes of a booster with categorical splits, for the CPU test-suite, which walks these
// arrays in Python the way the kernels of categorical.hip do: nodes = four 32-bit words per slot {bits, left, meta, size
// as float bits}, words = the sets kept beside the nodes, orig_id per slot, roots per tree.  info[0] = slots, [1] =
// words, [2] = trees, [3] = inline sets, [4] = sets in `words`; every array is written up to its cap (all caps 0: ask
// for the sizes).  Placement with the default layout, as a booster is uploaded.
int ohx_cat_flatten_cpu(const uint8_t* model, uint64_t model_len, uint32_t* nodes, uint64_t cap_slots, uint32_t* words,
                        uint64_t cap_words, int32_t* orig_id, uint32_t* roots, uint64_t cap_trees, uint64_t* info) {
  try {
    Forest f = load_model_buffer(model, (size_t)model_len);
    f.validate();
    const Placement p = place_forest(f, LayoutParams());
    const CatForest cf = emit_cat(f, p);
    info[0] = cf.nodes.size();
    info[1] = cf.words.size();
    info[2] = p.roots.size();
    info[3] = cf.inline_sets;
    info[4] = cf.word_sets;
    for (size_t i = 0; i < cf.nodes.size() && i < cap_slots; ++i) {
      memcpy(nodes + 4 * i, &cf.nodes[i], 16);
      orig_id[i] = cf.orig_id[i];
    }
    for (size_t i = 0; i < cf.words.size() && i < cap_words; ++i) words[i] = cf.words[i];
    for (size_t i = 0; i < p.roots.size() && i < cap_trees; ++i) roots[i] = p.roots[i];
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// The launch shapes of the selected-gridcells calls (cells.hpp): plan[0], plan[1] = blocks and items per block of an
// ordered pass over n items (the selection's box cells, the scatter's entries); plan[2] = floats between two lanes'
// rows in the gather's LDS tile; plan[3] = waves (blocks) of a gather of n cells.
int ohx_cells_plan(uint64_t n, uint32_t nfield, uint64_t* plan) {
  const CellsPassPlan p = plan_cells_pass(n);
  plan[0] = p.blocks;
  plan[1] = p.chunk;
  plan[2] = cells_gather_lds_stride(nfield);
  plan[3] = (n + kCellsWave - 1) / kCellsWave;
  return 0;
}

}  // extern "C"
#pragma GCC visibility pop
