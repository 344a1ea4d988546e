"""Synthetic inputs of SURVEY.md §8(d): feature batches and the synthetic OH booster.

The reference ships neither data nor a model (its models sit on NCCS paths,
``OH_GridComp/OH_instance_OH.rc:17-20``), so tests and the benchmark draw both from
``libohx_synth.so`` (host, g++) and ``libohx_synth_gpu.so`` (the same generator in HBM, hipcc);
both compile the same ``csrc/synth_common.h`` and agree bit for bit.  Neither is part of
the product library.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
SYNTH_LIB_PATH = os.path.join(_HERE, "lib", "libohx_synth.so")
SYNTH_GPU_LIB_PATH = os.path.join(_HERE, "lib", "libohx_synth_gpu.so")

FEATURE_SEED = 20241108
MODEL_SEED = 1060
NFEAT = 27
FEATURE_NAMES = ["LAT", "PL", "T", "NO2", "O3", "CH4", "CO", "ISOP", "ACET", "C2H6", "C3H8",
                 "PRPE", "ALK4", "MP", "H2O2", "TAUCLWDN", "TAUCLIDN", "TAUCLIUP", "TAUCLWUP",
                 "CLOUD", "QV", "GMISTRATO3", "ALBUV", "AODUP", "AODDN", "CH2O", "SZA"]
IS2D = [n in ("LAT", "GMISTRATO3", "ALBUV", "SZA") for n in FEATURE_NAMES]
PL_FEATURE = 1
XX_MISS = -999.0             # OH_GridCompMod.F90:213

# BASELINE.json configs: cubed-sphere C{n} is im = n, jm = 6n in MAPL's layout
GRIDS: Dict[str, Tuple[int, int, int]] = {
    "mock4x4": (4, 4, 72),
    "C12": (12, 72, 72),
    "C48": (48, 288, 72),
    "C90": (90, 540, 72),
    "C180": (180, 1080, 72),
    "C360": (360, 2160, 72),
    "C720L137": (720, 4320, 137),
}

_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(SYNTH_LIB_PATH):
            raise capi.OhxError(f"{SYNTH_LIB_PATH} is missing: run __graft_entry__.build()")
        lib = C.CDLL(SYNTH_LIB_PATH)
        lib.ohx_synth_last_error.restype = C.c_char_p
        lib.ohx_synth_rows_cpu.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.ohx_synth_field_cpu.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.ohx_synth_model.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                        C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.ohx_synth_free.argtypes = [C.c_void_p]
        lib.ohx_synth_set_threads.argtypes = [C.c_int]
        lib.ohx_model_convert.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_uint64)]
        lib.ohx_super_walk_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_float,
                                           C.c_void_p, C.POINTER(C.c_uint64)]
        lib.ohx_super_heads_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.ohx_super_walk_pack_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32,
                                                C.c_float, C.c_void_p, C.POINTER(C.c_uint64)]
        lib.ohx_super_records_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                              C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.ohx_super_line_count.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32,
                                             C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
        lib.ohx_contribs_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float, C.c_int,
                                         C.c_uint, C.c_void_p]
        lib.ohx_contribs_table_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.ohx_contribs_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
        lib.ohx_cells_plan.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.ohx_interactions_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float,
                                             C.c_int, C.c_uint, C.c_void_p]
        lib.ohx_interactions_table_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.ohx_interactions_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
        lib.ohx_cat_flatten_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                            C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.ohx_visits_layout.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        lib.ohx_visits_node_sums.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        lib.ohx_visits_refresh.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p]
        lib.ohx_visits_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_void_p,
                                        C.POINTER(C.c_uint64)]
        lib.ohx_refit_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                        C.c_void_p, C.POINTER(C.c_uint64)]
        lib.ohx_refit_write_back.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        lib.ohx_refit_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        lib.ohx_grow_node_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint64, C.c_float,
                                            C.c_float, C.c_uint64, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        lib.ohx_grow_append.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32] + [C.c_void_p] * 9 + [
            C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        lib.ohx_grow_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64),
                                      C.c_void_p]
        lib.ohx_grow_eval_stop.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        lib.ohx_grow_eval_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ohx_grow_eval_rmse.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
        lib.ohx_grow_eval_rmse.restype = C.c_double
        lib.ohx_grow_eval_plan.argtypes = [C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        lib.ohx_grow_node_split_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint64,
                                                     C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double), C.c_void_p,
                                                     C.c_void_p]
        lib.ohx_grow_solve_leaf_weighted.argtypes = [C.c_int64, C.c_uint64, C.c_float, C.c_float, C.c_void_p]
        lib.ohx_grow_solve_leaf_weighted.restype = None
        lib.ohx_grow_plan_weighted.argtypes = lib.ohx_grow_plan.argtypes
        lib.ohx_grow_weighted_rmse.argtypes = [C.c_void_p, C.c_uint64]
        lib.ohx_grow_weighted_rmse.restype = C.c_double
        lib.ohx_grow_weighted_compare.argtypes = [C.c_void_p, C.c_void_p]
        lib.ohx_grow_weighted_stop.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        lib.ohx_grow_bag.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_float, C.c_void_p, C.c_void_p]
        lib.ohx_grow_features.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        lib.ohx_grow_colsample_keys.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.ohx_grow_colsample_keys.restype = None
        lib.ohx_grow_colsample_pick.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float,
                                                C.c_void_p, C.c_void_p]
        lib.ohx_grow_colsample_has.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.ohx_grow_interact_parse.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ohx_grow_interact_allowed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.ohx_grow_interact_allowed.restype = None
        lib.ohx_grow_plan_sampled.argtypes = [C.c_uint64, C.c_uint32, C.c_float, C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p]
        lib.ohx_grow_deep_batch.argtypes = []
        lib.ohx_grow_deep_batch.restype = C.c_uint32
        lib.ohx_grow_plan_deep.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64),
                                           C.c_void_p, C.POINTER(C.c_uint64)]
        lib.ohx_grow_plan_deep_sampled.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int,
                                                   C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64)]
        lib.ohx_grow_deep_children.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                               C.POINTER(C.c_uint32)]
        lib.ohx_grow_pairs.argtypes = [C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_uint32)]
        lib.ohx_grow_pairs_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        lib.ohx_grow_reg_gain.argtypes = [C.c_int64, C.c_uint64, C.c_float, C.c_float, C.c_float]
        lib.ohx_grow_reg_gain.restype = C.c_double
        lib.ohx_grow_reg_leaf.argtypes = [C.c_int64, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
        lib.ohx_grow_reg_leaf.restype = None
        lib.ohx_grow_reg_node_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint64, C.c_float,
                                                C.c_float, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_double)]
        lib.ohx_grow_mono_weight.argtypes = [C.c_int64, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_double, C.c_double]
        lib.ohx_grow_mono_weight.restype = C.c_double
        lib.ohx_grow_mono_gain.argtypes = [C.c_int64, C.c_uint64, C.c_float, C.c_float, C.c_double]
        lib.ohx_grow_mono_gain.restype = C.c_double
        lib.ohx_grow_mono_leaf.argtypes = [C.c_int64, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_double,
                                           C.c_double, C.c_void_p]
        lib.ohx_grow_mono_leaf.restype = None
        lib.ohx_grow_mono_node_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint64, C.c_float,
                                                 C.c_float, C.c_float, C.c_float, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                                 C.POINTER(C.c_double), C.c_void_p]
        lib.ohx_grow_weighted_quantile.argtypes = [C.c_void_p, C.c_uint64]
        lib.ohx_grow_weighted_quantile.restype = C.c_double
        lib.ohx_grow_quantile_pick.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]
        lib.ohx_grow_quantile_leaves.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                                 C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ohx_grow_quantile_plan.argtypes = [C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        lib.ohx_grow_metric_row.argtypes = [C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.ohx_grow_weighted_mean.argtypes = [C.c_void_p, C.c_uint64]
        lib.ohx_grow_weighted_mean.restype = C.c_double
        lib.ohx_cuts_select.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_float, C.c_int, C.c_uint64, C.c_void_p,
                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.ohx_cuts_keys.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.ohx_cuts_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        lib.ohx_cluster_order.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_double)]
        lib.ohx_pick_level_period.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        lib.ohx_pick_level_period.restype = C.c_uint64
        _lib = lib
    return _lib


def set_threads(n: int) -> None:
    """Host threads the generators may use (torchrun pins OMP_NUM_THREADS=1 per rank)."""
    _load().ohx_synth_set_threads(int(n))


def _check(rc: int) -> None:
    if rc != 0:
        raise capi.OhxError(_load().ohx_synth_last_error().decode())


def rows_cpu(grid: Tuple[int, int, int], row_begin: int, nrows: int, seed: int = FEATURE_SEED) -> np.ndarray:
    """[nrows][27] float32, PL in hPa, rows m = i + im*(j + jm*k) (OH_GridCompMod.F90:309-345)."""
    im, jm, km = grid
    out = np.empty((nrows, NFEAT), dtype=np.float32)
    _check(_load().ohx_synth_rows_cpu(seed, im, jm, km, row_begin, nrows, out.ctypes.data))
    return out


def field_cpu(grid: Tuple[int, int, int], feature: int, seed: int = FEATURE_SEED) -> np.ndarray:
    """One MAPL field in Fortran order, returned as an [i,j(,k)]-indexed view.  feature -1 = TROPP (Pa); PL in Pa."""
    im, jm, km = grid
    two_d = feature < 0 or IS2D[feature]
    flat = np.empty(im * jm * (1 if two_d else km), dtype=np.float32)
    _check(_load().ohx_synth_field_cpu(seed, feature, im, jm, km, flat.ctypes.data))
    return flat.reshape((jm, im)).T if two_d else flat.reshape((km, jm, im)).transpose(2, 1, 0)


@dataclass
class SynthModel:
    image: np.ndarray          # uint8 file image (legacy binary or JSON)
    num_trees: int
    num_nodes: int
    num_leaves: int
    max_depth: int
    mean_path: float           # internal nodes visited per row per tree, over the growth sample


def _take(ptr: C.c_void_p, n: int) -> np.ndarray:
    lib = _load()
    buf = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n,)).copy()
    lib.ohx_synth_free(ptr)
    return buf


def make_model(num_trees: int = 100, max_depth: int = 18, sample_log2: int = 20, min_leaf: int = 8,
               grid: Tuple[int, int, int] = GRIDS["C90"], model_seed: int = MODEL_SEED,
               feature_seed: int = FEATURE_SEED, base_score: float = -13.0, leaf_sigma: float = 0.05,
               fmt: str = "binary") -> SynthModel:
    """The synthetic OH booster: `num_trees` trees of depth <= `max_depth`, 27 features,
    grown on 2**sample_log2 cells of `grid`, thresholds = sampled feature values."""
    lib = _load()
    out, n = C.c_void_p(), C.c_uint64()
    stats = (C.c_uint64 * 4)()
    im, jm, km = grid
    _check(lib.ohx_synth_model(model_seed, num_trees, max_depth, sample_log2, min_leaf, feature_seed, im, jm, km,
                               base_score, leaf_sigma, 1 if fmt == "json" else 0, C.byref(out), C.byref(n), stats))
    denom = float((1 << sample_log2) * max(num_trees, 1))
    return SynthModel(_take(out, n.value), num_trees, int(stats[0]), int(stats[1]), int(stats[2]),
                      float(stats[3]) / denom)


def convert_model(image, fmt: str) -> np.ndarray:
    """Legacy binary / JSON / UBJSON ("binary", "json", "ubj") through the product's own readers and
    writers (host logic)."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    out, n = C.c_void_p(), C.c_uint64()
    code = {"binary": 0, "json": 1, "ubj": 2}[fmt]
    _check(lib.ohx_model_convert(src.ctypes.data, src.nbytes, code, C.byref(out), C.byref(n)))
    return _take(out, n.value)


def cat_flatten_cpu(image):
    """What the flattening makes of a booster with categorical splits (csrc/flatten.hpp emit_cat), for tests that walk
    it on the host: dict of nodes uint32 [slots][4] = {bits, left, meta, size as float bits}, words uint32, orig_id
    int32 [slots], roots uint32 [trees], inline_sets, word_sets."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    info = (C.c_uint64 * 5)()
    _check(lib.ohx_cat_flatten_cpu(src.ctypes.data, src.nbytes, None, 0, None, 0, None, None, 0, info))
    slots, nwords, ntrees = int(info[0]), int(info[1]), int(info[2])
    nodes = np.zeros((slots, 4), dtype=np.uint32)
    words = np.zeros(max(nwords, 1), dtype=np.uint32)
    orig_id = np.zeros(slots, dtype=np.int32)
    roots = np.zeros(ntrees, dtype=np.uint32)
    _check(lib.ohx_cat_flatten_cpu(src.ctypes.data, src.nbytes, nodes.ctypes.data, slots, words.ctypes.data, nwords,
                                   orig_id.ctypes.data, roots.ctypes.data, ntrees, info))
    return {"nodes": nodes, "words": words[:nwords], "orig_id": orig_id, "roots": roots,
            "inline_sets": int(info[3]), "word_sets": int(info[4])}


SUPER_PACKS = (0, 1, 2, 3)   # csrc/flatten.hpp kSuperPack*: breadth first, + 128-byte tree bases, + sibling pairs, + families


def super_walk_cpu(image, rows: np.ndarray, missing: float = XX_MISS, super_pack=None):
    """Host check of the super-node layout the kernels read (csrc/flatten.hpp): emit_super's arrays walked
    the kernels' way - fixed trip count per tree, no finished state, fillers - by a scalar loop.  Test
    support, not a prediction path.  super_pack: the placement of the groups ("ohx_super_pack"; None = what a booster
    uploads by default).  Returns (margins, info) or (None, None) if the booster does not fit."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.empty(rows.shape[0], dtype=np.float32)
    info = (C.c_uint64 * 4)()
    if super_pack is None:
        rc = lib.ohx_super_walk_cpu(src.ctypes.data, src.nbytes, rows.ctypes.data, rows.shape[0], rows.shape[1], missing,
                                    out.ctypes.data, info)
    else:
        rc = lib.ohx_super_walk_pack_cpu(src.ctypes.data, src.nbytes, int(super_pack), rows.ctypes.data, rows.shape[0],
                                         rows.shape[1], missing, out.ctypes.data, info)
    if rc == 1:
        return None, None
    _check(rc)
    return out, {"super_nodes": int(info[0]), "phase1_trees": int(info[1]), "steps": int(info[2])}


def super_records_cpu(image, super_pack: int):
    """emit_super's arrays (csrc/flatten.hpp) for `super_pack`: dict of nodes uint32 [records][4] = {thr0, thrL, thrR as
    float bits, meta}, heads uint32 [trees][4] = {base, root_meta, root_thr bits, steps}, packed uint8 [trees] = the
    tree's deep groups were numbered by line.  None if the booster does not fit the super-node format."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    info = (C.c_uint64 * 2)()
    rc = lib.ohx_super_records_cpu(src.ctypes.data, src.nbytes, int(super_pack), None, 0, None, None, 0, info)
    if rc == 1:
        return None
    _check(rc)
    nodes = np.zeros((int(info[0]), 4), dtype=np.uint32)
    heads = np.zeros((int(info[1]), 4), dtype=np.uint32)
    packed = np.zeros(int(info[1]), dtype=np.uint8)
    _check(lib.ohx_super_records_cpu(src.ctypes.data, src.nbytes, int(super_pack), nodes.ctypes.data, nodes.shape[0],
                                     heads.ctypes.data, packed.ctypes.data, heads.shape[0], info))
    return {"nodes": nodes, "heads": heads, "packed": packed}


def super_line_count(image, tiles: np.ndarray, super_pack: int, brick=None, k_fastest: bool = True,
                     first_step: int = 4, missing: float = XX_MISS):
    """Distinct cache lines per deep gather of the super-node walk, counted on the host (csrc/line_count.cpp).  tiles:
    (ntile, 64, ncol) rows, a tile's 64 gridcells in grid order (i fastest, then j, then k inside the brick), 16
    consecutive tiles one block's; brick = (li, lj, lk) log2 extents of the brick a wave takes (None: 64 consecutive
    rows) and k_fastest its lane order, as the launch picks them.  Returns (table, info): table[step] = dict of means
    per wave-gather for the 0-based steps from first_step on that any tree has - records, lookups (64-byte blocks per
    quad, summed over the quads), lines (128 bytes), block_lines (128-byte lines per block of 16 tiles) - and the
    gathers counted; info = records of the forest, fillers among them, trees numbered by line."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    tiles = np.ascontiguousarray(tiles, dtype=np.float32)
    assert tiles.ndim == 3 and tiles.shape[1] == 64
    shape = np.array(list(brick) + [1 if k_fastest else 0] if brick else [0, 0, 0, 0], dtype=np.uint32)
    raw = np.zeros((32, 6), dtype=np.float64)
    info = (C.c_uint64 * 3)()
    rc = lib.ohx_super_line_count(src.ctypes.data, src.nbytes, int(super_pack), tiles.ctypes.data, tiles.shape[0],
                                  tiles.shape[2], missing, shape.ctypes.data, first_step, raw.ctypes.data, info)
    if rc == 1:
        return None, None
    _check(rc)
    table = {}
    for s in range(32):
        g, rec, look, lines, bg, bl = raw[s]
        if g > 0:
            table[s] = {"gathers": int(g), "records": rec / g, "lookups": look / g, "lines": lines / g,
                        "block_lines": bl / bg if bg > 0 else float("nan")}
    return table, {"records": int(info[0]), "fillers": int(info[1]), "packed_trees": int(info[2])}


def super_heads_cpu(image):
    """Per tree, what emit_super (csrc/flatten.cpp) made of it: an (ntrees, 2) uint32 array of (phase, steps) - phase 1
    when the root is evaluated from the head record, steps the walk's trip count.  Test support: which edge classes of
    the kernels a booster reaches.  None if the booster does not fit the super-node format."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    n = C.c_uint64()
    rc = lib.ohx_super_heads_cpu(src.ctypes.data, src.nbytes, None, 0, C.byref(n))
    if rc == 1:
        return None
    _check(rc)
    out = np.zeros((n.value, 2), dtype=np.uint32)
    _check(lib.ohx_super_heads_cpu(src.ctypes.data, src.nbytes, out.ctypes.data, n.value, C.byref(n)))
    return out


def cluster_order(agree, nrow: int):
    """What the product makes of the clustering pass's nine `agree` words over `nrow` rows (csrc/kernels.hpp
    cluster_order): (order, observed, by_chance, clustered) - rows of an order below kClusterOrderBelow are clustered."""
    words = np.ascontiguousarray(agree, dtype=np.uint32)
    assert words.shape == (9,)
    out = (C.c_double * 3)()
    on = _load().ohx_cluster_order(words.ctypes.data, int(nrow), out)
    return float(out[0]), float(out[1]), float(out[2]), bool(on)


def pick_level_period(verdict, kmax: int, nrow: int) -> int:
    """The level size the product adopts from the level search's verdict words (csrc/kernels.hpp pick_level_period):
    verdict[c][x] of four columns, x = 0 .. kmax - 2 for the periods nrow / (kmax - x).  0 = none."""
    words = np.ascontiguousarray(verdict, dtype=np.uint32).reshape(-1)
    assert kmax >= 2 and words.size == 4 * (kmax - 1)
    return int(_load().ohx_pick_level_period(words.ctypes.data, int(kmax), int(nrow)))


def contribs_cpu(image, rows: np.ndarray, num_feature: int, missing: float = XX_MISS, approximate: bool = False,
                 ntree_limit: int = 0) -> np.ndarray:
    """Host restatement of per-feature contributions (csrc/contribs_host.cpp: xgboost 1.6.0's recursive TreeShap or
    CalculateContributionsApprox, in float): (nrow, num_feature + 1) float32, column num_feature the bias.  Test
    support, the reference the GPU kernels are checked against."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.empty((rows.shape[0], num_feature + 1), dtype=np.float32)
    _check(lib.ohx_contribs_cpu(src.ctypes.data, src.nbytes, rows.ctypes.data, rows.shape[0], rows.shape[1], missing,
                                1 if approximate else 0, ntree_limit, out.ctypes.data))
    return out


def contribs_table_stats(image) -> Dict[str, int]:
    """Size of the exact mode's path table as the library builds it (csrc/contribs.cpp build_path_table)."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    st = (C.c_uint64 * 5)()
    _check(lib.ohx_contribs_table_stats(src.ctypes.data, src.nbytes, st))
    return {"bytes": int(st[0]), "paths": int(st[1]), "elements": int(st[2]), "sum_len1_sq": int(st[3]),
            "max_len": int(st[4])}


def contribs_plan(nrow: int, nfeat: int, ntree: int, allow_split: bool = True):
    """The launch shape OHXBoosterPredictContribs picks for a batch (csrc/contribs.cpp plan_contribs): (split, groups,
    trees_per_group, direct_launches) - direct_launches is exact mode's count of direct launches, 0 when split."""
    p = (C.c_uint64 * 4)()
    _check(_load().ohx_contribs_plan(nrow, nfeat, ntree, 1 if allow_split else 0, p))
    return bool(p[0]), int(p[1]), int(p[2]), int(p[3])


def _image(image) -> np.ndarray:
    return np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image


def visits_layout(image, max_trees: int = 1 << 16, max_leaves: int = 1 << 24):
    """The visit counts' maps of a booster (csrc/visits.hpp VisitForest) -> (tree_offsets[T + 1] uint64, leaf_offset[T + 1]
    uint32, leaf_node uint32): counter leaf_offset[t] + l belongs to file node leaf_node[leaf_offset[t] + l] of tree t."""
    img = _image(image)
    ntree = C.c_uint64()
    offs = np.zeros(max_trees + 1, dtype=np.uint64)
    loff = np.zeros(max_trees + 1, dtype=np.uint32)
    lnode = np.zeros(max_leaves, dtype=np.uint32)
    _check(_load().ohx_visits_layout(img.ctypes.data, img.nbytes, max_trees, max_leaves, C.byref(ntree), offs.ctypes.data,
                                     loff.ctypes.data, lnode.ctypes.data))
    T = ntree.value
    return offs[:T + 1].copy(), loff[:T + 1].copy(), lnode[:int(loff[T])].copy()


def visits_node_sums(image, leaf_counts) -> np.ndarray:
    """Leaf counters -> node counts in file numbering, tree after tree (what OHXBoosterGetVisitCounts does on the host)."""
    img = _image(image)
    offs, _, lnode = visits_layout(img)
    leaf_counts = np.ascontiguousarray(leaf_counts, dtype=np.uint64)
    out = np.full(int(offs[-1]), 0xDEADBEEF, dtype=np.uint64)
    _check(_load().ohx_visits_node_sums(img.ctypes.data, img.nbytes, leaf_counts.ctypes.data, leaf_counts.size,
                                        out.ctypes.data, out.size))
    return out


def visits_refresh(image, node_counts, prior_weight: float):
    """The covers OHXBoosterRefreshCover would store for these node counts -> (sum_hess float32 tree after tree, error):
    error is None, or the refusal's message - and sum_hess then the forest's covers as they are afterwards."""
    img = _image(image)
    node_counts = np.ascontiguousarray(node_counts, dtype=np.uint64)
    out = np.zeros(node_counts.size, dtype=np.float32)
    lib = _load()
    rc = lib.ohx_visits_refresh(img.ctypes.data, img.nbytes, node_counts.ctypes.data, node_counts.size, prior_weight,
                                out.ctypes.data)
    return out, (None if rc == 0 else lib.ohx_synth_last_error().decode())


def visits_plan(image, lds_leaves: int = 0, force_global: bool = False, num_cus: int = 256, ntiles: int = 1 << 20):
    """csrc/visits.hpp plan_visits for a booster -> dict: takes_lds (per tree), stage, hist_leaves, the two kernels'
    dynamic LDS bytes, capacity (leaves), and their blocks for `ntiles` tiles on `num_cus` CUs."""
    img = _image(image)
    T = len(visits_layout(img)[0]) - 1
    takes = np.zeros(max(T, 1), dtype=np.uint8)
    info = (C.c_uint64 * 8)()
    _check(_load().ohx_visits_plan(img.ctypes.data, img.nbytes, lds_leaves, int(force_global), num_cus, ntiles,
                                   takes.ctypes.data, info))
    return {"takes_lds": takes[:T].astype(bool), "stage": bool(info[0]), "hist_leaves": int(info[1]),
            "lds_bytes_lds": int(info[2]), "lds_bytes_global": int(info[3]), "capacity": int(info[4]),
            "lds_blocks": int(info[5]), "global_blocks": int(info[6]), "lds_trees": int(info[7])}


def refit_solve(G, H, eta: float, reg_lambda: float, unvisited: int, value, base_weight):
    """csrc/refit.cpp refit_solve on injected sums: G int64 and H uint64 per leaf, the old leaf tables ->
    (value, base_weight, leaves with H > 0) as OHXBoosterRefitLeaves would store them."""
    G = np.ascontiguousarray(G, dtype=np.int64)
    H = np.ascontiguousarray(H, dtype=np.uint64)
    v = np.array(value, dtype=np.float32)
    w = np.array(base_weight, dtype=np.float32)
    assert G.shape == H.shape == v.shape == w.shape and G.ndim == 1
    n = C.c_uint64()
    _check(_load().ohx_refit_solve(G.ctypes.data, H.ctypes.data, G.size, eta, reg_lambda, unvisited, v.ctypes.data,
                                   w.ctypes.data, C.byref(n)))
    return v, w, int(n.value)


def refit_write_back(image, value, base_weight):
    """csrc/refit.cpp refit_gather_leaves and refit_write_back on a booster: leaf tables in the dense numbering of
    visits_layout -> (old value table, old base_weight table, node values, node base_weights): the forest's arrays tree
    after tree in file numbering once the tables are written back."""
    img = _image(image)
    offs, loff, _ = visits_layout(img)
    value = np.ascontiguousarray(value, dtype=np.float32)
    base_weight = np.ascontiguousarray(base_weight, dtype=np.float32)
    nleaf, nnode = int(loff[-1]), int(offs[-1])
    assert value.size == nleaf and base_weight.size == nleaf
    ov, ob = np.zeros(max(nleaf, 1), dtype=np.float32), np.zeros(max(nleaf, 1), dtype=np.float32)
    nv, nb = np.zeros(max(nnode, 1), dtype=np.float32), np.zeros(max(nnode, 1), dtype=np.float32)
    _check(_load().ohx_refit_write_back(img.ctypes.data, img.nbytes, value.ctypes.data, base_weight.ctypes.data, nleaf,
                                        ov.ctypes.data, ob.ctypes.data, nv.ctypes.data, nb.ctypes.data, nnode))
    return ov[:nleaf], ob[:nleaf], nv[:nnode], nb[:nnode]


def refit_plan(nrow: int, num_feature: int = NFEAT, ntree: int = 1, num_cus: int = 256):
    """csrc/refit.hpp plan_refit -> dict: stage, lds_bytes, ids_blocks, accum_blocks, ids_bytes, block_rows (rows a
    block takes per trip of either kernel's loop), and the two kernels' block caps per CU."""
    info = (C.c_uint64 * 8)()
    _check(_load().ohx_refit_plan(nrow, num_feature, ntree, num_cus, info))
    return {"stage": bool(info[0]), "lds_bytes": int(info[1]), "ids_blocks": int(info[2]), "accum_blocks": int(info[3]),
            "ids_bytes": int(info[4]), "block_rows": int(info[5]), "ids_blocks_per_cu": int(info[6]),
            "accum_blocks_per_cu": int(info[7])}


def grow_node_split(G, H, cut_ptr, Gp: int, Hp: int, reg_lambda: float, gamma: float, min_child_rows: int):
    """csrc/grow.cpp grow_node_split (the shared grow_best_split per feature) on injected histograms G int64 / H uint64
    [num_feature][256] -> dict: valid, feature, j, default_left, splits, loss_chg (float64), GL, HL."""
    G = np.ascontiguousarray(G, dtype=np.int64)
    H = np.ascontiguousarray(H, dtype=np.uint64)
    cut_ptr = np.ascontiguousarray(cut_ptr, dtype=np.uint64)
    assert G.shape == H.shape and G.ndim == 2 and G.shape[1] == 256 and cut_ptr.size == G.shape[0] + 1
    loss = C.c_double()
    out, sums = np.zeros(5, dtype=np.uint32), np.zeros(2, dtype=np.int64)
    _check(_load().ohx_grow_node_split(G.ctypes.data, H.ctypes.data, G.shape[0], cut_ptr.ctypes.data, Gp, Hp, reg_lambda,
                                       gamma, min_child_rows, C.byref(loss), out.ctypes.data, sums.ctypes.data))
    return {"valid": bool(out[0]), "feature": int(out[1]), "j": int(out[2]), "default_left": int(out[3]),
            "splits": bool(out[4]), "loss_chg": float(loss.value), "GL": int(sums[0]), "HL": int(sums[1])}


def grow_append(image, tree, fmt: str = "json") -> np.ndarray:
    """csrc/grow.cpp grow_assemble_tree on node records (a dict of the nine arrays left, right, parent, feature,
    default_left, value, loss_chg, sum_hess, base_weight), appended to the booster of `image`; the longer forest in
    `fmt` ("binary", "json", "ubj")."""
    img = _image(image)
    n = len(tree["left"])
    arrs = [np.ascontiguousarray(tree[k], dtype=t) for k, t in (
        ("left", np.int32), ("right", np.int32), ("parent", np.int32), ("feature", np.uint32),
        ("default_left", np.uint32), ("value", np.float32), ("loss_chg", np.float32), ("sum_hess", np.float32),
        ("base_weight", np.float32))]
    assert all(a.size == n for a in arrs)
    out, m = C.c_void_p(), C.c_uint64()
    _check(_load().ohx_grow_append(img.ctypes.data, img.nbytes, n, *[a.ctypes.data for a in arrs],
                                   {"binary": 0, "json": 1, "ubj": 2}[fmt], C.byref(out), C.byref(m)))
    return _take(out, m.value)


def grow_plan(nrow: int, num_feature: int = NFEAT, ncuts: int = 0, max_depth: int = 6, num_cus: int = 256):
    """csrc/grow.hpp plan_grow -> dict: row_blocks and block_rows (bin, partition and leaf kernels), bin_lds_bytes,
    bins_bytes, hist_bytes, hist_block_rows, max_pairs, pair_bytes, and levels: per level a dict of slots, node_group,
    feat_group, node_groups, feat_groups, hist_blocks, lds_bytes."""
    info = (C.c_uint64 * 8)()
    lev = np.zeros((max(max_depth, 1), 7), dtype=np.uint64)
    _check(_load().ohx_grow_plan(nrow, num_feature, ncuts, max_depth, num_cus, info, lev.ctypes.data))
    names = ("slots", "node_group", "feat_group", "node_groups", "feat_groups", "hist_blocks", "lds_bytes")
    return {"row_blocks": int(info[0]), "block_rows": int(info[1]), "bin_lds_bytes": int(info[2]),
            "bins_bytes": int(info[3]), "hist_bytes": int(info[4]), "hist_block_rows": int(info[5]),
            "max_pairs": int(info[6]), "pair_bytes": int(info[7]),
            "levels": [dict(zip(names, (int(v) for v in row))) for row in lev]}


def boost_eval_stop(sums, patience: int):
    """csrc/grow.hpp grow_eval_stop, the stop rule of OHXBoosterBoostTreesEval, over the held-out sums after 0, 1, ...
    trees, each a pair (hi, lo) of uint64 with S = hi * 2^32 + lo (lo need not be below 2^32).
    -> (rounds_run, best_round)."""
    a = np.ascontiguousarray([[int(h), int(l)] for h, l in sums], dtype=np.uint64)
    out = np.zeros(2, dtype=np.uint32)
    _check(_load().ohx_grow_eval_stop(a.ctypes.data, len(a), patience, out.ctypes.data))
    return int(out[0]), int(out[1])


def boost_eval_compare(a, b):
    """csrc/grow.hpp grow_sum_less both ways and grow_sum_normal on sums (hi, lo) -> (-1 / 0 / 1, a normalised)."""
    a = np.ascontiguousarray([int(v) for v in a], dtype=np.uint64)
    b = np.ascontiguousarray([int(v) for v in b], dtype=np.uint64)
    normal = np.zeros(2, dtype=np.uint64)
    rc = _load().ohx_grow_eval_compare(a.ctypes.data, b.ctypes.data, normal.ctypes.data)
    return int(rc), (int(normal[0]), int(normal[1]))


def boost_eval_rmse(hi: int, lo: int, n: int) -> float:
    """csrc/grow.cpp grow_sum_rmse: sqrt((double)(hi * 2^32 + lo) * 2^-48 / n)."""
    return float(_load().ohx_grow_eval_rmse(hi, lo, n))


def grow_eval_plan(nrow: int, num_cus: int = 256):
    """csrc/grow.cpp plan_grow_eval_blocks -> dict: blocks of grow_sse_kernel and grow_walk_sse_kernel, block_rows."""
    info = (C.c_uint64 * 2)()
    _check(_load().ohx_grow_eval_plan(nrow, num_cus, info))
    return {"blocks": int(info[0]), "block_rows": int(info[1])}


def grow_node_split_weighted(G, H, cut_ptr, Gp: int, Hp: int, reg_lambda: float, gamma: float, min_child_weight: float):
    """csrc/grow.cpp grow_node_split_weighted (the shared grow_best_split_weighted per feature) on injected histograms
    G int64 / H uint64 (fixed-point hessian sums) [num_feature][256] -> dict as grow_node_split's; HL in fixed point."""
    G = np.ascontiguousarray(G, dtype=np.int64)
    H = np.ascontiguousarray(H, dtype=np.uint64)
    cut_ptr = np.ascontiguousarray(cut_ptr, dtype=np.uint64)
    assert G.shape == H.shape and G.ndim == 2 and G.shape[1] == 256 and cut_ptr.size == G.shape[0] + 1
    loss = C.c_double()
    out, sums = np.zeros(5, dtype=np.uint32), np.zeros(2, dtype=np.uint64)
    _check(_load().ohx_grow_node_split_weighted(G.ctypes.data, H.ctypes.data, G.shape[0], cut_ptr.ctypes.data, Gp, Hp,
                                                reg_lambda, gamma, min_child_weight, C.byref(loss), out.ctypes.data,
                                                sums.ctypes.data))
    return {"valid": bool(out[0]), "feature": int(out[1]), "j": int(out[2]), "default_left": int(out[3]),
            "splits": bool(out[4]), "loss_chg": float(loss.value), "GL": int(sums[:1].view(np.int64)[0]), "HL": int(sums[1])}


def grow_solve_leaf_weighted(G: int, H: int, eta: float, reg_lambda: float):
    """csrc/grow.hpp grow_solve_leaf_weighted and grow_hess -> (leaf value, base_weight, sum_hess) as float32."""
    out = np.zeros(3, dtype=np.float32)
    _load().ohx_grow_solve_leaf_weighted(G, H, eta, reg_lambda, out.ctypes.data)
    return out[0], out[1], out[2]


def grow_plan_weighted(nrow: int, num_feature: int = NFEAT, ncuts: int = 0, max_depth: int = 6, num_cus: int = 256):
    """csrc/grow.hpp plan_grow_weighted -> the dict of grow_plan, for the 16-byte bins of the weighted histogram kernel."""
    info = (C.c_uint64 * 8)()
    lev = np.zeros((max(max_depth, 1), 7), dtype=np.uint64)
    _check(_load().ohx_grow_plan_weighted(nrow, num_feature, ncuts, max_depth, num_cus, info, lev.ctypes.data))
    names = ("slots", "node_group", "feat_group", "node_groups", "feat_groups", "hist_blocks", "lds_bytes")
    return {"row_blocks": int(info[0]), "block_rows": int(info[1]), "bin_lds_bytes": int(info[2]),
            "bins_bytes": int(info[3]), "hist_bytes": int(info[4]), "hist_block_rows": int(info[5]),
            "max_pairs": int(info[6]), "pair_bytes": int(info[7]),
            "levels": [dict(zip(names, (int(v) for v in row))) for row in lev]}


def grow_deep_batch() -> int:
    """csrc/grow.hpp kGrowDeepBatch: the node slots whose histograms a batch of a deep level holds."""
    return int(_load().ohx_grow_deep_batch())


def grow_plan_deep(nrow: int, num_feature: int = NFEAT, ncuts: int = 0, max_depth: int = 12, num_cus: int = 256):
    """csrc/grow.hpp plan_grow_deep -> the dict of grow_plan_weighted over the min(max_depth, 8) levels kept in LDS, and
    for the levels from 8 on: batch, deep_hist_blocks, deep_block_rows, scratch_bytes (a batch's histograms; 0 up to
    depth 8), best_bytes (a level's candidates) and node_stride (node records of one round)."""
    info = (C.c_uint64 * 8)()
    deep = (C.c_uint64 * 6)()
    lev = np.zeros((max(min(max_depth, 8), 1), 7), dtype=np.uint64)
    _check(_load().ohx_grow_plan_deep(nrow, num_feature, ncuts, max_depth, num_cus, info, lev.ctypes.data, deep))
    names = ("slots", "node_group", "feat_group", "node_groups", "feat_groups", "hist_blocks", "lds_bytes")
    return {"row_blocks": int(info[0]), "block_rows": int(info[1]), "bin_lds_bytes": int(info[2]),
            "bins_bytes": int(info[3]), "hist_bytes": int(info[4]), "hist_block_rows": int(info[5]),
            "max_pairs": int(info[6]), "pair_bytes": int(info[7]),
            "levels": [dict(zip(names, (int(v) for v in row))) for row in lev],
            "batch": int(deep[0]), "deep_hist_blocks": int(deep[1]), "deep_block_rows": int(deep[2]),
            "scratch_bytes": int(deep[3]), "best_bytes": int(deep[4]), "node_stride": int(deep[5])}


def grow_plan_deep_sampled(nrow: int, num_feature: int = NFEAT, n_sel: int = NFEAT, ncuts: int = 0, max_depth: int = 12,
                           num_cus: int = 256):
    """csrc/grow.hpp plan_grow_deep_sampled -> the dict of grow_plan_deep over the n_sel features a tree of
    OHXBoosterBoostTreesDeepSampled sees (levels, hist_bytes, scratch_bytes and best_bytes count n_sel columns), with
    bins_bytes the planes of all num_feature features, and n_sel."""
    info = (C.c_uint64 * 8)()
    deep = (C.c_uint64 * 6)()
    lev = np.zeros((max(min(max_depth, 8), 1), 7), dtype=np.uint64)
    _check(_load().ohx_grow_plan_deep_sampled(nrow, num_feature, n_sel, ncuts, max_depth, num_cus, info, lev.ctypes.data, deep))
    names = ("slots", "node_group", "feat_group", "node_groups", "feat_groups", "hist_blocks", "lds_bytes")
    return {"row_blocks": int(info[0]), "block_rows": int(info[1]), "bin_lds_bytes": int(info[2]),
            "bins_bytes": int(info[3]), "hist_bytes": int(info[4]), "hist_block_rows": int(info[5]),
            "max_pairs": int(info[6]), "pair_bytes": int(info[7]),
            "levels": [dict(zip(names, (int(v) for v in row))) for row in lev],
            "batch": int(deep[0]), "deep_hist_blocks": int(deep[1]), "deep_block_rows": int(deep[2]),
            "scratch_bytes": int(deep[3]), "best_bytes": int(deep[4]), "node_stride": int(deep[5]), "n_sel": int(n_sel)}


def grow_deep_children(flags, width: int, next_id: int):
    """csrc/grow.hpp grow_chunked_children: the left-child ids a block of `width` lanes hands the open nodes of a level
    with these split flags, walking them in chunks with a running total -> (left uint32 [count], 0 where a node does
    not split; the number of splits)."""
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    left = np.zeros(max(f.size, 1), dtype=np.uint32)
    n = C.c_uint32()
    _check(_load().ohx_grow_deep_children(f.ctypes.data, f.size, width, next_id, left.ctypes.data, C.byref(n)))
    return left[:f.size], int(n.value)


GROW_OBJECTIVES = {"squarederror": 0, "pseudohuber": 1, "quantile": 2}
GROW_FLAG_LABEL, GROW_FLAG_WEIGHT = 1, 8   # csrc/grow.hpp kGrowFlagLabel, kGrowFlagWeight


def ohx_grow_pairs(objective: str, slope: float, pred, y, w=None):
    """csrc/grow.hpp grow_pair over the rows: the fixed-point (gradient, hessian) pair of every row by `objective`
    ("squarederror", "pseudohuber" with `slope`, or "quantile" with alpha in the slope's place) -> (q int64 [n], hq uint32 [n], flags).  A row that raises a flag
    (GROW_FLAG_LABEL, GROW_FLAG_WEIGHT) has the pair (0, 0).  w None: every weight is 1."""
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    assert pred.shape == y.shape and pred.ndim == 1
    wa = None if w is None else np.ascontiguousarray(w, dtype=np.float32)
    assert wa is None or wa.shape == y.shape
    q = np.zeros(max(y.size, 1), dtype=np.int64)
    hq = np.zeros(max(y.size, 1), dtype=np.uint32)
    flags = C.c_uint32()
    _check(_load().ohx_grow_pairs(GROW_OBJECTIVES[objective], float(slope), pred.ctypes.data, y.ctypes.data,
                                  None if wa is None else wa.ctypes.data, y.size, q.ctypes.data, hq.ctypes.data, C.byref(flags)))
    return q[:y.size], hq[:y.size], int(flags.value)


def grow_pairs_plan(nrow: int, num_feature: int, ncuts: int, max_depth: int, num_cus: int):
    """The pair planes in the plan of a call (csrc/grow.hpp GrowPlan.pairs_bytes) -> {"pairs_bytes", "row_bytes"}."""
    info = (C.c_uint64 * 2)()
    _check(_load().ohx_grow_pairs_plan(nrow, num_feature, ncuts, max_depth, num_cus, info))
    return {"pairs_bytes": int(info[0]), "row_bytes": int(info[1])}


GROW_METRICS = {"rmse": 0, "mae": 1, "pseudohuber": 2, "quantile": 3}


def ohx_grow_reg_gain(G: int, H: int, reg_lambda: float, reg_alpha: float, max_delta_step: float) -> float:
    """csrc/grow.hpp GrowRegHess.gain: the regularised gain of a node's fixed-point sums, a double."""
    return float(_load().ohx_grow_reg_gain(int(G), int(H), reg_lambda, reg_alpha, max_delta_step))


def ohx_grow_reg_leaf(G: int, H: int, eta: float, reg_lambda: float, reg_alpha: float, max_delta_step: float):
    """csrc/grow.hpp GrowRegHess.solve_leaf -> (leaf, base_weight, sum_hess) float32."""
    out = np.zeros(3, dtype=np.float32)
    _load().ohx_grow_reg_leaf(int(G), int(H), eta, reg_lambda, reg_alpha, max_delta_step, out.ctypes.data)
    return out[0], out[1], out[2]


def grow_reg_node_split(Gh, Hh, cut_ptr, Gp: int, Hp: int, reg_lambda: float, min_child_weight: float, reg_alpha: float,
                        max_delta_step: float):
    """csrc/grow.hpp grow_node_split with GrowRegHess over the histograms Gh int64 / Hh uint64 [F][256] -> None or
    (loss_chg, f, j, dl, GL, HL)."""
    Gh = np.ascontiguousarray(Gh, dtype=np.int64)
    Hh = np.ascontiguousarray(Hh, dtype=np.uint64)
    ptr = np.ascontiguousarray(cut_ptr, dtype=np.uint64)
    assert Gh.shape == Hh.shape and Gh.shape[1] == 256 and len(ptr) == Gh.shape[0] + 1
    out = np.zeros(4, dtype=np.uint64)
    loss = C.c_double()
    _check(_load().ohx_grow_reg_node_split(Gh.ctypes.data, Hh.ctypes.data, Gh.shape[0], ptr.ctypes.data, int(Gp), int(Hp), reg_lambda,
                                           min_child_weight, reg_alpha, max_delta_step, out.ctypes.data, C.byref(loss)))
    if not int(out[0]):
        return None
    key = int(out[1])
    return float(loss.value), key >> 9, (key >> 1) & 255, key & 1, int(out[2:3].view(np.int64)[0]), int(out[3])


def ohx_grow_mono_weight(G: int, H: int, reg_lambda: float, reg_alpha: float, max_delta_step: float, lo: float, hi: float) -> float:
    """csrc/grow.hpp GrowMonoHess.weight: the regularised weight of a node's fixed-point sums clamped into (lo, hi), a double."""
    return float(_load().ohx_grow_mono_weight(int(G), int(H), reg_lambda, reg_alpha, max_delta_step, lo, hi))


def ohx_grow_mono_gain(G: int, H: int, reg_lambda: float, reg_alpha: float, w: float) -> float:
    """csrc/grow.hpp grow_gain_at: gain_w of a node's fixed-point sums at the weight w, a double."""
    return float(_load().ohx_grow_mono_gain(int(G), int(H), reg_lambda, reg_alpha, w))


def ohx_grow_mono_leaf(G: int, H: int, eta: float, reg_lambda: float, reg_alpha: float, max_delta_step: float, lo: float, hi: float):
    """csrc/grow.hpp GrowMonoHess.solve_leaf under the interval (lo, hi) -> (leaf, base_weight, sum_hess) float32."""
    out = np.zeros(3, dtype=np.float32)
    _load().ohx_grow_mono_leaf(int(G), int(H), eta, reg_lambda, reg_alpha, max_delta_step, lo, hi, out.ctypes.data)
    return out[0], out[1], out[2]


def grow_mono_node_split(Gh, Hh, cut_ptr, Gp: int, Hp: int, reg_lambda: float, min_child_weight: float, reg_alpha: float,
                         max_delta_step: float, lo: float, hi: float, constraints):
    """csrc/grow.hpp grow_mono_node_split over the histograms Gh int64 / Hh uint64 [F][256], the node's interval (lo, hi) and
    the F constraints -> None or (loss_chg, f, j, dl, GL, HL, (lo_L, hi_L, lo_R, hi_R))."""
    Gh = np.ascontiguousarray(Gh, dtype=np.int64)
    Hh = np.ascontiguousarray(Hh, dtype=np.uint64)
    ptr = np.ascontiguousarray(cut_ptr, dtype=np.uint64)
    con = np.ascontiguousarray(constraints, dtype=np.int8)
    assert Gh.shape == Hh.shape and Gh.shape[1] == 256 and len(ptr) == Gh.shape[0] + 1 and con.shape == (Gh.shape[0],)
    out = np.zeros(4, dtype=np.uint64)
    children = np.zeros(4, dtype=np.float64)
    loss = C.c_double()
    _check(_load().ohx_grow_mono_node_split(Gh.ctypes.data, Hh.ctypes.data, Gh.shape[0], ptr.ctypes.data, int(Gp), int(Hp), reg_lambda,
                                            min_child_weight, reg_alpha, max_delta_step, lo, hi, con.ctypes.data, out.ctypes.data,
                                            C.byref(loss), children.ctypes.data))
    if not int(out[0]):
        return None
    key = int(out[1])
    return (float(loss.value), key >> 9, (key >> 1) & 255, key & 1, int(out[2:3].view(np.int64)[0]), int(out[3]),
            tuple(float(v) for v in children))


def ohx_grow_metric_row(metric: str, slope: float, pred, y):
    """csrc/grow.hpp grow_metric_row over the rows: what a row adds to S beside its hq by `metric` ("rmse", "mae" or
    "pseudohuber" with `slope`, or "quantile" with alpha in the slope's place) -> (sq uint64 [n], sound bool [n]); a refused
    residual has sq = 0."""
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    assert pred.shape == y.shape and pred.ndim == 1
    sq = np.zeros(max(y.size, 1), dtype=np.uint64)
    sound = np.zeros(max(y.size, 1), dtype=np.uint8)
    _check(_load().ohx_grow_metric_row(GROW_METRICS[metric], float(slope), pred.ctypes.data, y.ctypes.data, y.size, sq.ctypes.data,
                                       sound.ctypes.data))
    return sq[:y.size], sound[:y.size].astype(bool)


def boost_weighted_mean(p2: int, p1: int, p0: int, W: int) -> float:
    """csrc/grow.cpp grow_wide_mean: ((double)(p2 * 2^64 + p1 * 2^32 + p0) * 2^-48) / ((double)W * 2^-24)."""
    s = np.ascontiguousarray([p2, p1, p0], dtype=np.uint64)
    return float(_load().ohx_grow_weighted_mean(s.ctypes.data, W))


def boost_weighted_quantile(p2: int, p1: int, p0: int, W: int) -> float:
    """csrc/grow.cpp grow_wide_quantile: ((double)(p2 * 2^64 + p1 * 2^32 + p0) * 2^-72) / ((double)W * 2^-24)."""
    s = np.ascontiguousarray([p2, p1, p0], dtype=np.uint64)
    return float(_load().ohx_grow_weighted_quantile(s.ctypes.data, W))


def grow_quantile_pick(bins, pass_: int, alpha: float, prefix: int = 0, below: int = 0, W: int = 0):
    """csrc/grow_quantile.hpp grow_quantile_pick: one pass's pick over a leaf's 256 bins (uint64) from the leaf's state
    (prefix, below, W; pass 0 makes W from the bins) -> None where the leaf holds no weight, else (prefix, below, W)."""
    b = np.ascontiguousarray(bins, dtype=np.uint64)
    assert b.shape == (256,)
    st = np.array([prefix, below, W], dtype=np.uint64)
    rc = _load().ohx_grow_quantile_pick(b.ctypes.data, int(pass_), float(alpha), st.ctypes.data)
    return None if rc == 0 else (int(st[0]), int(st[1]), int(st[2]))


def grow_quantile_leaves(pos, hq, pred, y, leaves, alpha: float, eta: float = 1.0):
    """The whole per-leaf select on the host, pass by pass as the device runs it (csrc/grow_host.cpp over
    grow_quantile.hpp): rows at node pos[r] (uint16) with hessian hq[r] (uint32) and residual y[r] - pred[r]; `leaves` the
    node ids in slot order -> (found bool [L], key uint32 [L], value float32 [L], W uint64 [L]); a leaf without weight is
    not found."""
    pos = np.ascontiguousarray(pos, dtype=np.uint16)
    hq = np.ascontiguousarray(hq, dtype=np.uint32)
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    lv = np.ascontiguousarray(leaves, dtype=np.uint16)
    assert pos.shape == hq.shape == pred.shape == y.shape and pos.ndim == 1 and lv.ndim == 1
    L = max(lv.size, 1)
    found = np.zeros(L, dtype=np.uint8)
    key = np.zeros(L, dtype=np.uint32)
    value = np.zeros(L, dtype=np.float32)
    W = np.zeros(L, dtype=np.uint64)
    _check(_load().ohx_grow_quantile_leaves(pos.ctypes.data, hq.ctypes.data, pred.ctypes.data, y.ctypes.data, y.size, lv.ctypes.data,
                                            lv.size, float(alpha), float(eta), found.ctypes.data, key.ctypes.data, value.ctypes.data,
                                            W.ctypes.data))
    return found[:lv.size].astype(bool), key[:lv.size], value[:lv.size], W[:lv.size]


def grow_quantile_plan(nrow: int, max_depth: int = 6, num_cus: int = 256):
    """csrc/grow_quantile.hpp plan_grow_quantile, the grid launch_grow_tree_quantile gives grow_quantile_pass_kernel -> dict:
    pass_blocks (over the rows) and pass_block_rows (rows such a block takes per trip), group (leaves a block holds), groups
    (leaf groups, the grid's second dimension) and row_blocks (grow_plan_weighted's, which the blocks are cut from)."""
    info = (C.c_uint64 * 5)()
    _check(_load().ohx_grow_quantile_plan(nrow, max_depth, num_cus, info))
    return {"pass_blocks": int(info[0]), "pass_block_rows": int(info[1]), "group": int(info[2]), "groups": int(info[3]),
            "row_blocks": int(info[4])}


def boost_weighted_rmse(p2: int, p1: int, p0: int, W: int) -> float:
    """csrc/grow.cpp grow_wide_rmse: sqrt(((double)(p2 * 2^64 + p1 * 2^32 + p0) * 2^-72) / ((double)W * 2^-24))."""
    s = np.ascontiguousarray([p2, p1, p0], dtype=np.uint64)
    return float(_load().ohx_grow_weighted_rmse(s.ctypes.data, W))


def boost_weighted_compare(a, b) -> int:
    """csrc/grow.hpp grow_sum_less on wide sums (p2, p1, p0), both ways -> -1 / 0 / 1."""
    a = np.ascontiguousarray([int(v) for v in a], dtype=np.uint64)
    b = np.ascontiguousarray([int(v) for v in b], dtype=np.uint64)
    return int(_load().ohx_grow_weighted_compare(a.ctypes.data, b.ctypes.data))


def boost_weighted_stop(sums, patience: int):
    """csrc/grow.hpp grow_eval_stop over wide sums (p2, p1, p0) after 0, 1, ... trees -> (rounds_run, best_round)."""
    a = np.ascontiguousarray([[int(v) for v in s] for s in sums], dtype=np.uint64)
    out = np.zeros(2, dtype=np.uint32)
    _check(_load().ohx_grow_weighted_stop(a.ctypes.data, len(a), patience, out.ctypes.data))
    return int(out[0]), int(out[1])


def boost_bag(seed: int, tree: int, nrow: int, subsample: float):
    """csrc/grow.hpp grow_row_key, grow_in_bag and grow_sample_threshold: the bag of tree `tree` (its index in the whole
    forest) over rows 0 .. nrow - 1 -> (bool [nrow], k_s).  Raises where the subsample is one the call refuses."""
    out = np.zeros(max(nrow, 1), dtype=np.uint8)
    ks = C.c_uint32()
    _check(_load().ohx_grow_bag(int(seed) & 0xFFFFFFFFFFFFFFFF, int(tree) & 0xFFFFFFFFFFFFFFFF, nrow, subsample, out.ctypes.data,
                                C.addressof(ks)))
    return out[:nrow].astype(bool), int(ks.value)


def boost_features(seed: int, tree: int, F: int, colsample: float):
    """csrc/grow.cpp grow_pick_features: the features tree `tree` may split on, ascending (uint8 [n_sel])."""
    out = np.zeros(max(F, 1), dtype=np.uint8)
    n = C.c_uint32()
    _check(_load().ohx_grow_features(int(seed) & 0xFFFFFFFFFFFFFFFF, int(tree) & 0xFFFFFFFFFFFFFFFF, F, colsample, out.ctypes.data,
                                     C.addressof(n)))
    return out[:int(n.value)].copy()


_U64 = 0xFFFFFFFFFFFFFFFF


def colsample_keys(seed: int, tree: int, level: int, node: int):
    """csrc/grow.hpp grow_level_key and grow_node_key over grow_col_key -> (K_lvl(tree, level), K_node(tree, node))."""
    keys = np.zeros(2, dtype=np.uint64)
    _load().ohx_grow_colsample_keys(int(seed) & _U64, int(tree) & _U64, level, node, keys.ctypes.data)
    return int(keys[0]), int(keys[1])


def _colsample_pick(which: int, seed: int, tree: int, at: int, features, fraction: float):
    lst = np.ascontiguousarray(features, dtype=np.uint8)
    out = np.zeros(max(len(lst), 1), dtype=np.uint8)
    n = C.c_uint32()
    _check(_load().ohx_grow_colsample_pick(which, int(seed) & _U64, int(tree) & _U64, at, lst.ctypes.data, len(lst), fraction,
                                           out.ctypes.data, C.addressof(n)))
    return out[:int(n.value)].copy()


def boost_level_features(seed: int, tree: int, level: int, tree_list, bylevel: float):
    """csrc/grow.cpp grow_pick_level_features: what level `level` of tree `tree` keeps of the tree's list (uint8 [n_lvl])."""
    return _colsample_pick(0, seed, tree, level, tree_list, bylevel)


def boost_node_features(seed: int, tree: int, node: int, level_list, bynode: float):
    """csrc/grow.cpp grow_pick_node_features: what node `node` of tree `tree` keeps of its level's list (uint8 [n_node])."""
    return _colsample_pick(1, seed, tree, node, level_list, bynode)


def boost_node_has_feature(seed: int, tree: int, node: int, level_list, n_node: int, f: int) -> bool:
    """csrc/grow.hpp grow_node_has_feature: the rank the split kernels compute; f must be in the level's list."""
    lst = np.ascontiguousarray(level_list, dtype=np.uint8)
    return bool(_load().ohx_grow_colsample_has(int(seed) & _U64, int(tree) & _U64, node, lst.ctypes.data, len(lst), n_node, f))


def _feature_set(words) -> set:
    return {64 * k + b for k in (0, 1) for b in range(64) if (int(words[k]) >> b) & 1}


def _feature_words(features):
    w = [0, 0]
    for f in features:
        w[int(f) >> 6] |= 1 << (int(f) & 63)
    return w


def interact_parse(value: str, num_feature: int):
    """csrc/grow.cpp grow_interact_parse and grow_interact_active -> (the groups as sorted lists of feature ids, whether
    they are active for a booster of num_feature features); raises RuntimeError where the grammar refuses the value."""
    words = np.zeros(128, dtype=np.uint64)
    n, active = C.c_uint32(), C.c_int()
    _check(_load().ohx_grow_interact_parse(value.encode(), num_feature, words.ctypes.data, C.addressof(n), C.addressof(active)))
    return [sorted(_feature_set(words[2 * g:2 * g + 2])) for g in range(int(n.value))], bool(active.value)


def interact_allowed(path, groups, num_feature: int) -> set:
    """csrc/grow.hpp grow_interact_allowed: the features a node may split on whose path has split on `path`."""
    P = np.array(_feature_words(path), dtype=np.uint64)
    gw = np.array([w for g in groups for w in _feature_words(g)] or [0, 0], dtype=np.uint64)
    out = np.zeros(2, dtype=np.uint64)
    _load().ohx_grow_interact_allowed(P.ctypes.data, gw.ctypes.data, len(groups), num_feature, out.ctypes.data)
    return _feature_set(out)


def grow_plan_sampled(nrow: int, num_feature: int = NFEAT, colsample: float = 1.0, ncuts: int = 0, max_depth: int = 6,
                      num_cus: int = 256):
    """The level plan of OHXBoosterBoostTreesSampled: csrc/grow.hpp plan_grow_weighted over the n_sel features a tree
    sees -> the dict of grow_plan_weighted with n_sel; bins_bytes are the planes of all num_feature features."""
    info = (C.c_uint64 * 9)()
    lev = np.zeros((max(max_depth, 1), 7), dtype=np.uint64)
    _check(_load().ohx_grow_plan_sampled(nrow, num_feature, colsample, ncuts, max_depth, num_cus, info, lev.ctypes.data))
    names = ("slots", "node_group", "feat_group", "node_groups", "feat_groups", "hist_blocks", "lds_bytes")
    return {"row_blocks": int(info[0]), "block_rows": int(info[1]), "bin_lds_bytes": int(info[2]),
            "bins_bytes": int(info[3]), "hist_bytes": int(info[4]), "hist_block_rows": int(info[5]),
            "max_pairs": int(info[6]), "pair_bytes": int(info[7]), "n_sel": int(info[8]),
            "levels": [dict(zip(names, (int(v) for v in row))) for row in lev]}


def quantile_cuts_select(x, missing: float = float("nan"), max_bins: int = 255, row_step: int = 1, bits=(12, 10, 10)):
    """csrc/cuts.cpp cuts_select_host: the radix select of OHXDMatrixQuantileCuts on the host, over rows 0, row_step, ...
    of the row-major `x` - the counting is a plain loop, the step between passes and the final assembly are the code
    the product library runs.  bits: the key bits each pass takes (they sum to 32).
    -> (cut_ptr uint64 [ncol + 1], cut_values float32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.ndim == 2
    nrow, ncol = x.shape
    b = np.ascontiguousarray(bits, dtype=np.uint32)
    cut_ptr = np.zeros(ncol + 1, dtype=np.uint64)
    cap = ncol * 254
    values = np.zeros(max(cap, 1), dtype=np.float32)
    needed = C.c_uint64()
    _check(_load().ohx_cuts_select(x.ctypes.data, nrow, ncol, missing, max_bins, row_step, b.ctypes.data, b.size,
                                   cut_ptr.ctypes.data, values.ctypes.data, cap, C.byref(needed)))
    return cut_ptr, values[:needed.value].copy()


def cuts_keys(bits):
    """csrc/cuts.hpp cuts_key of float32 bit patterns (uint32) and cuts_unkey of the keys -> (keys, back)."""
    u = np.ascontiguousarray(bits, dtype=np.uint32)
    keys, back = np.zeros_like(u), np.zeros_like(u)
    _check(_load().ohx_cuts_keys(u.ctypes.data, u.size, keys.ctypes.data, back.ctypes.data))
    return keys, back


def cuts_plan(nrow: int, row_step: int = 1, ncol: int = NFEAT, num_cus: int = 256):
    """csrc/cuts.hpp plan_cuts -> dict: sampled (rows), block_rows, pass 1's blocks1, col_group1, col_groups1 and
    lds1_bytes, passes 2 and 3's blocks, col_group, col_groups and lds_bytes (the staged prefixes), table1_bytes and
    table_bytes."""
    info = (C.c_uint64 * 12)()
    _check(_load().ohx_cuts_plan(nrow, row_step, ncol, num_cus, info))
    names = ("sampled", "blocks1", "col_group1", "col_groups1", "lds1_bytes", "blocks", "col_group", "col_groups",
             "lds_bytes", "table1_bytes", "table_bytes", "block_rows")
    return dict(zip(names, (int(v) for v in info)))


def cells_plan(n: int, nfield: int = 27):
    """The launch shapes of the selected-gridcells calls (csrc/cells.hpp): (blocks, items_per_block) of an ordered pass
    over `n` items - the selection's box cells, the scatter's list entries - then the gather's LDS lane stride in
    floats for `nfield` fields and its waves for `n` cells."""
    p = (C.c_uint64 * 4)()
    _check(_load().ohx_cells_plan(n, nfield, p))
    return int(p[0]), int(p[1]), int(p[2]), int(p[3])


def interactions_cpu(image, rows: np.ndarray, num_feature: int, missing: float = XX_MISS, approximate: bool = False,
                     ntree_limit: int = 0) -> np.ndarray:
    """Host restatement of SHAP interaction values (csrc/contribs_host.cpp: xgboost 1.6.0's
    PredictInteractionContributions, in float): (nrow, num_feature + 1, num_feature + 1) float32, index num_feature
    the bias.  2 * num_feature + 3 TreeSHAP passes per row.  Test support."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.empty((rows.shape[0], num_feature + 1, num_feature + 1), dtype=np.float32)
    _check(lib.ohx_interactions_cpu(src.ctypes.data, src.nbytes, rows.ctypes.data, rows.shape[0], rows.shape[1],
                                    missing, 1 if approximate else 0, ntree_limit, out.ctypes.data))
    return out


def interactions_table_stats(image) -> Dict[str, int]:
    """Exact interactions' feature-path index size and the path sums (d = distinct features of a path)."""
    lib = _load()
    src = np.frombuffer(bytes(image), dtype=np.uint8) if not isinstance(image, np.ndarray) else image
    st = (C.c_uint64 * 5)()
    _check(lib.ohx_interactions_table_stats(src.ctypes.data, src.nbytes, st))
    return {"index_bytes": int(st[0]), "paths": int(st[1]), "sum_d": int(st[2]), "sum_d2": int(st[3]),
            "sum_d3": int(st[4])}


def interactions_plan(nrow: int, nfeat: int, ntree: int, allow_split: bool = True):
    """The launch shape OHXBoosterPredictInteractions picks for exact mode (csrc/contribs.cpp plan_interactions):
    (split, groups, trees_per_group, direct_launches, part_floats) - direct_launches 0 when split."""
    p = (C.c_uint64 * 5)()
    _check(_load().ohx_interactions_plan(nrow, nfeat, ntree, 1 if allow_split else 0, p))
    return bool(p[0]), int(p[1]), int(p[2]), int(p[3]), int(p[4])


# ---- device generators (torch tensors in HBM; libohx_synth_gpu.so, test support like the rest of this file) ----

_gpu_lib = None


def _load_gpu():
    global _gpu_lib
    if _gpu_lib is None:
        if not os.path.exists(SYNTH_GPU_LIB_PATH):
            raise capi.OhxError(f"{SYNTH_GPU_LIB_PATH} is missing: run __graft_entry__.build()")
        lib = C.CDLL(SYNTH_GPU_LIB_PATH)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        lib.ohx_synth_gpu_last_error.restype = C.c_char_p
        lib.ohx_synth_rows_device.argtypes = [u32, i32, i32, i32, u64, u64, vp, vp]
        lib.ohx_synth_field_device.argtypes = [u32, i32, i32, i32, i32, vp, vp]
        lib.ohx_inject_missing_device.argtypes = [vp, u64, u32, u32, C.c_float, vp]
        lib.ohx_probe_cluster_keys.argtypes = [vp, u64, vp, u32, u32, vp, u64, u32, C.c_float, u32, u32, u32, vp, vp, vp,
                                               i32, vp]
        lib.ohx_probe_sort_pairs.argtypes = [vp, vp, vp, vp, u64, u32, vp, C.POINTER(i32), C.POINTER(u64)]
        lib.ohx_probe_detect_period.argtypes = [vp, u64, u32, vp, u32, u32, vp, vp]
        _gpu_lib = lib
    return _gpu_lib


def _check_gpu(rc: int) -> None:
    if rc != 0:
        raise capi.OhxError(_load_gpu().ohx_synth_gpu_last_error().decode())


def rows_device(grid: Tuple[int, int, int], row_begin: int, nrows: int, out, seed: int = FEATURE_SEED,
                stream: int = 0) -> None:
    """Fill torch tensor `out` ([nrows][27] float32, on the GPU) with rows row_begin.."""
    im, jm, km = grid
    assert out.is_contiguous() and out.numel() == nrows * NFEAT
    _check_gpu(_load_gpu().ohx_synth_rows_device(seed, im, jm, km, row_begin, nrows, out.data_ptr(), stream or None))


def field_device(grid: Tuple[int, int, int], feature: int, out, seed: int = FEATURE_SEED, stream: int = 0) -> None:
    im, jm, km = grid
    _check_gpu(_load_gpu().ohx_synth_field_device(seed, feature, im, jm, km, out.data_ptr(), stream or None))


def inject_missing_device(rows, rate_per_million: int, missing: float = XX_MISS, seed: int = 7, stream: int = 0) -> None:
    _check_gpu(_load_gpu().ohx_inject_missing_device(rows.data_ptr(), rows.numel(), seed, rate_per_million, missing,
                                                     stream or None))


# ---- probes of the clustering pass and the level search (csrc/probe_gpu.hip): the product's kernels on the test's buffers ----

def probe_cluster_keys(nodes, heads, num_feature: int, rows, ncol: int, missing: float, ntrees: int, nsteps: int,
                       zorder: int, keys, vals, agree, num_cus: int, stream: int = 0, nrow=None) -> None:
    """launch_cluster_keys (csrc/kernels.hip) on torch tensors in HBM: `nodes` ([records][4] uint32-sized words) and
    `heads` ([trees][4]) are super_records_cpu's arrays uploaded as they are, `rows` holds nrow x ncol float32, `keys`
    and `vals` take nrow words each, `agree` is nine words that must be zero before.  Raises OhxError where the
    launcher refuses."""
    nrow = rows.numel() // max(ncol, 1) if nrow is None else nrow
    assert rows.numel() >= nrow * ncol and keys.numel() >= nrow and vals.numel() >= nrow and agree.numel() >= 9
    assert all(t.is_contiguous() and t.element_size() == 4 for t in (nodes, heads, rows, keys, vals, agree))
    assert nodes.numel() % 4 == 0 and heads.numel() % 4 == 0
    _check_gpu(_load_gpu().ohx_probe_cluster_keys(nodes.data_ptr(), nodes.numel() * 4, heads.data_ptr(), heads.numel() // 4,
                                                  num_feature, rows.data_ptr(), nrow, ncol, missing, ntrees, nsteps,
                                                  zorder, keys.data_ptr(), vals.data_ptr(), agree.data_ptr(), num_cus,
                                                  stream or None))


def probe_sort_pairs(keys_a, keys_b, vals_a, vals_b, n: int, key_bits: int, stream: int = 0):
    """sort_pairs_u32 (csrc/sort_pairs.hip) called the way the clustering pass calls it, on torch tensors of n 32-bit
    words each; the stream has run on return.  -> (which, temp_bytes): vals_a (0) or vals_b (1) holds the result."""
    assert all(t.is_contiguous() and t.element_size() == 4 and t.numel() >= n for t in (keys_a, keys_b, vals_a, vals_b))
    which, temp = C.c_int(-1), C.c_uint64(0)
    _check_gpu(_load_gpu().ohx_probe_sort_pairs(keys_a.data_ptr(), keys_b.data_ptr(), vals_a.data_ptr(), vals_b.data_ptr(),
                                                n, key_bits, stream or None, C.byref(which), C.byref(temp)))
    return which.value, temp.value


def probe_detect_period(data, nrow: int, ncol: int, cols, kmax: int, verdict, stream: int = 0) -> None:
    """launch_detect_period (csrc/kernels.hip) on torch tensors: `data` nrow x ncol float32, `verdict` len(cols) x
    (kmax - 1) words that must be zero before; verdict[c][x] is then 0, 1 or 2 for the period nrow / (kmax - x)."""
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    assert 1 <= cols.size <= 4 and data.numel() >= nrow * ncol and verdict.numel() >= cols.size * max(kmax - 1, 0)
    assert data.is_contiguous() and verdict.is_contiguous() and data.element_size() == 4 and verdict.element_size() == 4
    _check_gpu(_load_gpu().ohx_probe_detect_period(data.data_ptr(), nrow, ncol, cols.ctypes.data, cols.size, kmax,
                                                   verdict.data_ptr(), stream or None))


def run1_state(grid, seed=17):
    """A synthetic OH import state for OHXBoosterRun1: physically plausible magnitudes, arbitrary values."""
    im, jm, km = grid
    rng = np.random.default_rng(seed)
    f32 = np.float32

    def u(lo, hi, shape):
        return (lo + (hi - lo) * rng.random(shape)).astype(f32)
    ps = u(6.0e4, 1.04e5, (im, jm))
    sig = (np.arange(km + 1, dtype=f32) / f32(km)) ** 2
    ple = (f32(1.0) + (ps[:, :, None] - f32(1.0)) * sig[None, None, :]).astype(f32)         # Pa, edges 0..km
    zle = (f32(8.0e4) * (f32(1.0) - sig[None, None, :]) * u(0.9, 1.1, (im, jm))[:, :, None]).astype(f32)
    vol, plane = (im, jm, km), (im, jm)
    cloudy = rng.random(vol) < 0.25
    st = {
        "ple_mod": ple, "ple_bst": (ple * u(0.98, 1.02, (im, jm))[:, :, None]).astype(f32), "zle_bst": zle,
        "t_mod": u(190, 310, vol), "q_mod": u(1e-7, 2e-2, vol), "tropp_mod": u(9.0e3, 3.0e4, plane),
        "tauclw": np.where(cloudy, u(0, 8, vol), 0).astype(f32), "taucli": np.where(~cloudy & (rng.random(vol) < 0.2), u(0, 3, vol), 0).astype(f32),
        "scacoef": [u(0, 5e-6, vol) for _ in range(7)],
        "gmito3": u(250, 450, plane), "gmitto3": u(20, 60, plane),
        "lat_deg": u(-90, 90, plane), "t_bst": u(190, 310, vol), "cloud": np.clip(u(-0.5, 1.0, vol), 0, 1).astype(f32),
        "qv": u(1e-7, 2e-2, vol), "albuv": u(0.02, 0.9, plane), "sza": u(0, 113, plane),
        "default_oh": u(1e-15, 5e-13, vol),
    }
    for name, lo in (("no2", 1e-12), ("o3", 1e-8), ("ch4", 1.6e-6), ("co", 2e-8), ("isop", 1e-14), ("acet", 1e-11),
                     ("c2h6", 1e-11), ("c3h8", 1e-12), ("prpe", 1e-13), ("alk4", 1e-12), ("mp", 1e-11), ("h2o2", 1e-11),
                     ("ch2o", 1e-12)):
        st[name] = (f32(lo) * np.exp2(u(0, 8, vol))).astype(f32)
    return st
