"""ctypes binding of libohxgb.so (include/ohxgb.h) — plumbing only.

The names mirror the reference's Fortran binding module
(``Shared/xgb_fortran_api.F90``): the same eleven XGBoost C-API symbols, plus the
device-resident / fused extensions.  Nothing here computes; every numeric result
comes out of the HIP kernels in the shared library, and loading fails loudly if
the library has not been built.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libohxgb.so")
# the library's default of "ohx_ring_rounds" (csrc/kernels.hpp LaunchTuning::ring_rounds; tests/test_capi_host.py pins it)
RING_ROUNDS_DEFAULT = 64
RING_ROUNDS_NO_GRID = 16      # kRingRoundsNoGrid: at most, for rows not known to lie on a grid
RING_ROUNDS_PERMUTED = 4      # kRingRoundsPermuted: at most, for rows that come through the clustering pass
# visit counts (csrc/visits.hpp): a block is 4 waves of 64 rows and strides over the tiles; blocks of one launch per CU at
# most - the LDS kernel's per tree - so one trip of a kernel's loop is CUs x this x 256 rows
VISITS_BLOCK_ROWS = 256
VISITS_LDS_BLOCKS_PER_CU = 1
VISITS_GLOBAL_BLOCKS_PER_CU = 4

# every symbol include/ohxgb.h declares
ABI_SYMBOLS = [
    "XGBGetLastError", "XGDMatrixCreateFromMat", "XGDMatrixFree", "XGDMatrixNumRow", "XGDMatrixNumCol",
    "XGDMatrixSaveBinary", "XGDMatrixCreateFromFile", "XGBoosterCreate", "XGBoosterFree", "XGBoosterLoadModel",
    "XGBoosterSaveModel", "XGBoosterLoadModelFromBuffer", "XGBoosterPredict", "XGBoosterSetParam",
    "OHXDeviceCount", "OHXDMatrixCreateFromDevice", "OHXDMatrixSetGrid", "OHXDMatrixGetGrid", "OHXDMatrixInferGrid", "OHXBoosterPredictDevice", "OHXBoosterCheck",
    "OHXBoosterPredictContribs", "OHXBoosterPredictContribsDevice",
    "OHXBoosterPredictInteractions", "OHXBoosterPredictInteractionsDevice",
    "OHXBoosterPredictContribsFields", "OHXBoosterPredictContribsFieldsDevice",
    "OHXBoosterCountVisits", "OHXBoosterCountVisitsDevice", "OHXBoosterGetVisitCounts", "OHXBoosterResetVisitCounts",
    "OHXBoosterRefreshCover", "OHXBoosterRefitLeaves", "OHXBoosterRefitLeavesDevice",
    "OHXBoosterBoostTrees", "OHXBoosterBoostTreesDevice", "OHXBoosterBoostTreesEval", "OHXBoosterBoostTreesEvalDevice",
    "OHXBoosterBoostTreesWeighted", "OHXBoosterBoostTreesWeightedDevice",
    "OHXBoosterBoostTreesSampled", "OHXBoosterBoostTreesSampledDevice",
    "OHXBoosterBoostTreesDeep", "OHXBoosterBoostTreesDeepDevice",
    "OHXBoosterBoostTreesDeepSampled", "OHXBoosterBoostTreesDeepSampledDevice",
    "OHXQuantileCuts", "OHXDMatrixQuantileCuts",
    "OHXSelectCells", "OHXSelectCellsDevice", "OHXGatherCells", "OHXGatherCellsDevice",
    "OHXScatterCells", "OHXScatterCellsDevice",
    "OHXBoosterPredictFields", "OHXBoosterPredictFieldsDevice", "OHXBoosterRun1", "OHXBoosterRun1Device", "OHXOHPostProcess", "OHXOHPostProcessDevice",
    "OHXJulianDay", "OHXSolarGeometry", "OHXSolarGeometryDevice", "OHXBoosterGetInfo", "OHXBoosterGetNumGroups", "OHXBoosterGetNumCategoricalSplits", "OHXBoosterKernelSymbol", "OHXBoosterKernelSymbolRows",
    "OHXBoosterRingReruns", "OHXBoosterCopyEngineChoice", "OHXUnregisterHost", "OHXReleaseScratch",
    "OHXCommGetUniqueId", "OHXCommInitRank", "OHXCommFree", "OHXCommInfo", "OHXShardRows", "OHXAllGatherOH",
]
# the subset QuickChem's xgb_fortran_api binds (Shared/xgb_fortran_api.F90:19-119)
REFERENCE_BOUND_SYMBOLS = [
    "XGBoosterLoadModel", "XGBoosterSaveModel", "XGDMatrixSaveBinary", "XGDMatrixFree", "XGDMatrixCreateFromFile",
    "XGBoosterPredict", "XGBoosterCreate", "XGDMatrixCreateFromMat", "XGDMatrixNumRow", "XGDMatrixNumCol",
    "XGBoosterFree",
]


class OhxError(RuntimeError):
    pass


class OHXRun1Args(C.Structure):
    """struct OHXRun1Args of include/ohxgb.h (part 3)."""
    _P = C.c_void_p
    _fields_ = ([("im", C.c_int32), ("jm", C.c_int32), ("km", C.c_int32), ("dynamic_k_range", C.c_int32),
                 ("tropp_min", C.c_float), ("ohscale", C.c_float), ("missing", C.c_float),
                 ("avogad", C.c_float), ("runiv", C.c_float), ("epsilon", C.c_float)] +
                [(n, C.c_void_p) for n in ("ple_mod", "t_mod", "q_mod", "tropp_mod", "ple_bst", "zle_bst", "tauclw",
                                           "taucli")] +
                [("scacoef", C.c_void_p * 7)] +
                [(n, C.c_void_p) for n in ("gmito3", "gmitto3", "lat_deg", "t_bst", "no2", "o3", "ch4", "co", "isop",
                                           "acet", "c2h6", "c3h8", "prpe", "alk4", "mp", "h2o2", "cloud", "qv", "albuv",
                                           "ch2o", "sza", "default_oh", "oh", "oh_boost", "ndwet", "k1", "k2",
                                           "diag_pl_bst", "diag_tauclwdn", "diag_tauclidn", "diag_taucliup",
                                           "diag_tauclwup", "diag_aodup", "diag_aoddn", "diag_aod", "diag_strato3")])

RUN1_DIAG_3D = ["diag_pl_bst", "diag_tauclwdn", "diag_tauclidn", "diag_taucliup", "diag_tauclwup", "diag_aodup",
                "diag_aoddn", "diag_aod"]


RUN1_INPUTS_3D = ["t_mod", "q_mod", "tauclw", "taucli", "t_bst", "no2", "o3", "ch4", "co", "isop", "acet", "c2h6", "c3h8",
                  "prpe", "alk4", "mp", "h2o2", "cloud", "qv", "ch2o", "default_oh"]
RUN1_INPUTS_EDGE = ["ple_mod", "ple_bst", "zle_bst"]
RUN1_INPUTS_2D = ["tropp_mod", "gmito3", "gmitto3", "lat_deg", "albuv", "sza"]


_lib: Optional[C.CDLL] = None


def declare_xgb_api(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes for the XGBoost C-API subset (shared with the CPU oracle library)."""
    vp, u64, f32, i32 = C.c_void_p, C.c_uint64, C.c_float, C.c_int
    lib.XGBGetLastError.restype = C.c_char_p
    lib.XGBGetLastError.argtypes = []
    lib.XGDMatrixCreateFromMat.argtypes = [vp, u64, u64, f32, C.POINTER(vp)]
    lib.XGDMatrixFree.argtypes = [vp]
    lib.XGDMatrixNumRow.argtypes = [vp, C.POINTER(u64)]
    lib.XGDMatrixNumCol.argtypes = [vp, C.POINTER(u64)]
    lib.XGDMatrixSaveBinary.argtypes = [vp, C.c_char_p, i32]
    lib.XGDMatrixCreateFromFile.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    lib.XGBoosterCreate.argtypes = [vp, u64, C.POINTER(vp)]
    lib.XGBoosterFree.argtypes = [vp]
    lib.XGBoosterLoadModel.argtypes = [vp, C.c_char_p]
    lib.XGBoosterSaveModel.argtypes = [vp, C.c_char_p]
    lib.XGBoosterLoadModelFromBuffer.argtypes = [vp, vp, u64]
    lib.XGBoosterPredict.argtypes = [vp, vp, i32, C.c_uint, i32, C.POINTER(u64), C.POINTER(C.POINTER(f32))]
    return lib


def load_library(path: str = LIB_PATH) -> C.CDLL:
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise OhxError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    lib = declare_xgb_api(C.CDLL(path))
    vp, u64, f32, i32, u32 = C.c_void_p, C.c_uint64, C.c_float, C.c_int, C.c_uint32
    lib.XGBoosterSetParam.argtypes = [vp, C.c_char_p, C.c_char_p]
    lib.OHXDeviceCount.argtypes = [C.POINTER(i32)]
    lib.OHXDMatrixCreateFromDevice.argtypes = [vp, u64, u64, f32, C.POINTER(vp)]
    lib.OHXDMatrixSetGrid.argtypes = [vp, i32, i32, u64]
    lib.OHXDMatrixGetGrid.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u64), C.POINTER(i32)]
    lib.OHXDMatrixInferGrid.argtypes = [vp, vp, C.POINTER(i32)]
    lib.OHXBoosterPredictDevice.argtypes = [vp, vp, i32, C.c_uint, vp, vp]
    lib.OHXBoosterCheck.argtypes = [vp, vp]
    lib.OHXBoosterPredictContribs.argtypes = [vp, vp, i32, C.c_uint, C.POINTER(u64), C.POINTER(C.POINTER(f32))]
    lib.OHXBoosterPredictContribsDevice.argtypes = [vp, vp, i32, C.c_uint, vp, vp]
    lib.OHXBoosterPredictInteractions.argtypes = [vp, vp, i32, C.c_uint, C.POINTER(u64), C.POINTER(C.POINTER(f32))]
    lib.OHXBoosterPredictInteractionsDevice.argtypes = [vp, vp, i32, C.c_uint, vp, vp]
    lib.OHXBoosterPredictContribsFields.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32), i32, i32, i32, i32, i32,
                                                    i32, i32, f32, i32, C.c_uint, C.POINTER(vp)]
    lib.OHXBoosterPredictContribsFieldsDevice.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32), i32, i32, i32, i32,
                                                          i32, i32, i32, f32, i32, C.c_uint, C.POINTER(vp), vp]
    lib.OHXBoosterCountVisits.argtypes = [vp, vp]
    lib.OHXBoosterCountVisitsDevice.argtypes = [vp, vp, vp]
    lib.OHXBoosterGetVisitCounts.argtypes = [vp, vp, C.POINTER(u64), C.POINTER(C.POINTER(u64)), C.POINTER(C.POINTER(u64)),
                                             C.POINTER(u64)]
    lib.OHXBoosterResetVisitCounts.argtypes = [vp]
    lib.OHXBoosterRefreshCover.argtypes = [vp, vp, f32]
    lib.OHXBoosterRefitLeaves.argtypes = [vp, vp, vp, u64, f32, f32, i32, C.POINTER(u64)]
    lib.OHXBoosterRefitLeavesDevice.argtypes = [vp, vp, vp, u64, f32, f32, i32, C.POINTER(u64), vp]
    lib.OHXBoosterBoostTrees.argtypes = [vp, vp, vp, u64, vp, vp, i32, i32, f32, f32, f32, u64, C.POINTER(u64)]
    lib.OHXBoosterBoostTreesDevice.argtypes = [vp, vp, vp, u64, vp, vp, i32, i32, f32, f32, f32, u64, C.POINTER(u64), vp]
    lib.OHXBoosterBoostTreesEval.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, i32, i32, f32, f32, f32, u64, i32, vp, vp,
                                             C.POINTER(i32), C.POINTER(i32), C.POINTER(u64)]
    lib.OHXBoosterBoostTreesEvalDevice.argtypes = lib.OHXBoosterBoostTreesEval.argtypes + [vp]
    lib.OHXBoosterBoostTreesWeighted.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, i32, i32, f32, f32, f32, f32,
                                                 i32, vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u64)]
    lib.OHXBoosterBoostTreesWeightedDevice.argtypes = lib.OHXBoosterBoostTreesWeighted.argtypes + [vp]
    lib.OHXBoosterBoostTreesDeep.argtypes = lib.OHXBoosterBoostTreesWeighted.argtypes
    lib.OHXBoosterBoostTreesDeepDevice.argtypes = lib.OHXBoosterBoostTreesWeightedDevice.argtypes
    lib.OHXBoosterBoostTreesSampled.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, i32, i32, f32, f32, f32, f32,
                                                f32, f32, u64, i32, vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u64)]
    lib.OHXBoosterBoostTreesSampledDevice.argtypes = lib.OHXBoosterBoostTreesSampled.argtypes + [vp]
    lib.OHXBoosterBoostTreesDeepSampled.argtypes = lib.OHXBoosterBoostTreesSampled.argtypes
    lib.OHXBoosterBoostTreesDeepSampledDevice.argtypes = lib.OHXBoosterBoostTreesSampledDevice.argtypes
    lib.OHXQuantileCuts.argtypes = [vp, u64, u64, f32, i32, vp, vp, u64, C.POINTER(u64)]
    lib.OHXDMatrixQuantileCuts.argtypes = [vp, u64, i32, vp, vp, u64, C.POINTER(u64), vp]
    lib.OHXBoosterPredictFields.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32), i32, i32, i32, i32, i32, i32, i32,
                                            f32, i32, f32, vp, vp]
    i64 = C.c_int64
    lib.OHXSelectCells.argtypes = [i32] * 9 + [vp, i32, vp, i32, f32, vp, i64, C.POINTER(i64)]
    lib.OHXSelectCellsDevice.argtypes = [i32] * 9 + [vp, i32, vp, i32, f32, vp, i64, vp, vp, vp]
    lib.OHXGatherCells.argtypes = [C.POINTER(vp), C.POINTER(C.c_int32), i32, i32, i32, i32, i32, vp, i64, vp]
    lib.OHXGatherCellsDevice.argtypes = [C.POINTER(vp), C.POINTER(C.c_int32), i32, i32, i32, i32, i32, vp, i64, vp, vp, vp]
    lib.OHXScatterCells.argtypes = [vp, i64, i64, vp, i64, vp, i32, i32, i32]
    lib.OHXScatterCellsDevice.argtypes = [vp, i64, i64, vp, i64, vp, i32, i32, i32, vp, vp]
    lib.OHXBoosterPredictFieldsDevice.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32), i32, i32, i32, i32, i32,
                                                  i32, i32, f32, i32, f32, vp, vp, vp]
    lib.OHXBoosterRun1.argtypes = [vp, C.POINTER(OHXRun1Args)]
    lib.OHXBoosterRun1Device.argtypes = [vp, C.POINTER(OHXRun1Args), vp]
    lib.OHXOHPostProcess.argtypes = [i32, i32, i32, f32, f32, f32] + [vp] * 8
    lib.OHXOHPostProcessDevice.argtypes = [i32, i32, i32, f32, f32, f32] + [vp] * 9
    lib.OHXJulianDay.argtypes = [i32, C.POINTER(i32)]
    lib.OHXSolarGeometry.argtypes = [i32, vp, vp, i32, i32, f32, f32, vp, vp]
    lib.OHXSolarGeometryDevice.argtypes = [i32, vp, vp, i32, i32, f32, f32, vp, vp, vp]
    lib.OHXBoosterGetInfo.argtypes = [vp, C.POINTER(u64)]
    lib.OHXBoosterGetNumGroups.argtypes = [vp, C.POINTER(u64)]
    lib.OHXBoosterGetNumCategoricalSplits.argtypes = [vp, C.POINTER(u64)]
    lib.OHXBoosterKernelSymbol.argtypes = [vp, u64, C.POINTER(C.c_char_p)]
    lib.OHXBoosterKernelSymbolRows.argtypes = [vp, vp, C.POINTER(C.c_char_p)]
    lib.OHXBoosterRingReruns.argtypes = [vp, vp, C.POINTER(u64)]
    lib.OHXBoosterCopyEngineChoice.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    lib.OHXUnregisterHost.argtypes = [vp]
    lib.OHXReleaseScratch.argtypes = []
    lib.OHXCommGetUniqueId.argtypes = [vp]
    lib.OHXCommInitRank.argtypes = [vp, i32, i32, C.POINTER(vp)]
    lib.OHXCommFree.argtypes = [vp]
    lib.OHXCommInfo.argtypes = [C.POINTER(i32)]
    lib.OHXShardRows.argtypes = [u64, i32, i32, C.POINTER(u64), C.POINTER(u64)]
    lib.OHXAllGatherOH.argtypes = [vp, vp, u64, u64, vp, vp]
    if path == LIB_PATH:
        _lib = lib
    return lib


def check(lib: C.CDLL, rc: int) -> None:
    if rc != 0:
        raise OhxError(lib.XGBGetLastError().decode("utf-8", "replace"))


def _as_f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


# MAPL_DEGREES_TO_RADIANS / MAPL_RADIANS_TO_DEGREES as MAPL defines them (real32 of pi / 180 and its inverse)
DEG2RAD = np.float32(np.float32(np.pi) / np.float32(180.0))
RAD2DEG = np.float32(np.float32(180.0) / np.float32(np.pi))


def julian_day(nymd: int, lib: Optional[C.CDLL] = None) -> int:
    """OHXJulianDay: day of year of a yyyymmdd date (OH_GridCompMod.F90:1905-1936)."""
    lib = lib or load_library()
    out = C.c_int32()
    check(lib, lib.OHXJulianDay(nymd, C.byref(out)))
    return out.value


def solar_geometry(jday: int, lats, lons, deg2rad=DEG2RAD, rad2deg=RAD2DEG, lib: Optional[C.CDLL] = None):
    """OHXSolarGeometry on [i,j]-indexed (im, jm) arrays in radians -> (lat_deg, sza_noon), same indexing."""
    lib = lib or load_library()
    la = np.ascontiguousarray(np.asarray(lats, dtype=np.float32).T)
    lo = np.ascontiguousarray(np.asarray(lons, dtype=np.float32).T)
    jm, im = la.shape
    lat_deg, sza = np.empty_like(la), np.empty_like(la)
    check(lib, lib.OHXSolarGeometry(jday, la.ctypes.data, lo.ctypes.data, im, jm, float(deg2rad), float(rad2deg),
                                    lat_deg.ctypes.data, sza.ctypes.data))
    return lat_deg.T, sza.T


class DMatrix:
    """XGDMatrixCreateFromMat / OHXDMatrixCreateFromDevice handle."""

    def __init__(self, data=None, missing: float = float("nan"), *, device_ptr: int = 0, nrow: int = 0, ncol: int = 0,
                 lib: Optional[C.CDLL] = None):
        self.lib = lib or load_library()
        self.handle = C.c_void_p()
        if data is not None:
            arr = _as_f32(data)
            if arr.ndim != 2:
                raise ValueError("data must be 2-D [nrow][ncol]")
            nrow, ncol = arr.shape
            check(self.lib, self.lib.XGDMatrixCreateFromMat(arr.ctypes.data, nrow, ncol, missing, C.byref(self.handle)))
        else:
            check(self.lib, self.lib.OHXDMatrixCreateFromDevice(device_ptr, nrow, ncol, missing, C.byref(self.handle)))

    @property
    def num_row(self) -> int:
        out = C.c_uint64()
        check(self.lib, self.lib.XGDMatrixNumRow(self.handle, C.byref(out)))
        return out.value

    @property
    def num_col(self) -> int:
        out = C.c_uint64()
        check(self.lib, self.lib.XGDMatrixNumCol(self.handle, C.byref(out)))
        return out.value

    def set_grid(self, im: int, jm: int, row0: int = 0) -> "DMatrix":
        """OHXDMatrixSetGrid: the rows are rows row0.. of the (im, jm, *) gather (speed only)."""
        check(self.lib, self.lib.OHXDMatrixSetGrid(self.handle, im, jm, row0))
        return self

    def infer_grid(self, stream: int = 0) -> bool:
        """OHXDMatrixInferGrid: look for the level size in the rows (device matrices; waits for `stream`)."""
        found = C.c_int32()
        check(self.lib, self.lib.OHXDMatrixInferGrid(self.handle, stream or None, C.byref(found)))
        return bool(found.value)

    def grid(self):
        """OHXDMatrixGetGrid -> (im, jm, row0, inferred)."""
        im, jm, r0, inf = C.c_int32(), C.c_int32(), C.c_uint64(), C.c_int32()
        check(self.lib, self.lib.OHXDMatrixGetGrid(self.handle, C.byref(im), C.byref(jm), C.byref(r0), C.byref(inf)))
        return im.value, jm.value, r0.value, bool(inf.value)

    def quantile_cuts(self, row_step: int = 1, max_bins: int = 255, stream=None, pad_to: Optional[int] = None):
        """OHXDMatrixQuantileCuts -> (cut_ptr uint64, cut_values float32): the cuts quantile_cuts makes from rows 0,
        row_step, 2 * row_step, ... of this matrix, found on the GPU where the rows lie (`stream`: the stream they are
        ready on; the call waits).  cut_ptr has num_col + 1 entries; pad_to=F repeats the last one up to F + 1 entries,
        for a booster of F features that the matrix has fewer columns than."""
        ncol = self.num_col
        cut_ptr = np.zeros(ncol + 1, dtype=np.uint64)
        cap = ncol * (max_bins - 1) if 2 <= max_bins <= 255 else 0
        values = np.zeros(max(cap, 1), dtype=np.float32)
        needed = C.c_uint64()
        check(self.lib, self.lib.OHXDMatrixQuantileCuts(self.handle, row_step, max_bins, cut_ptr.ctypes.data,
                                                        values.ctypes.data, cap, C.byref(needed), stream or None))
        if pad_to is not None and pad_to > ncol:
            cut_ptr = np.concatenate([cut_ptr, np.full(pad_to - ncol, cut_ptr[-1], dtype=np.uint64)])
        return cut_ptr, values[:needed.value].copy()

    def save_binary(self, fname: str) -> None:
        check(self.lib, self.lib.XGDMatrixSaveBinary(self.handle, fname.encode(), 1))

    @classmethod
    def from_file(cls, fname: str, lib: Optional[C.CDLL] = None) -> "DMatrix":
        self = cls.__new__(cls)
        self.lib = lib or load_library()
        self.handle = C.c_void_p()
        check(self.lib, self.lib.XGDMatrixCreateFromFile(fname.encode(), 1, C.byref(self.handle)))
        return self

    def free(self) -> None:
        if self.handle:
            check(self.lib, self.lib.XGDMatrixFree(self.handle))
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Booster:
    """XGBoosterCreate / LoadModel / Predict handle."""

    def __init__(self, model_file: Optional[str] = None, *, model_buffer: Optional[bytes] = None,
                 lib: Optional[C.CDLL] = None):
        self.lib = lib or load_library()
        self.handle = C.c_void_p()
        # as the reference does: a handle by value and len == 0 (OH_GridCompMod.F90:255-256)
        check(self.lib, self.lib.XGBoosterCreate(None, 0, C.byref(self.handle)))
        if model_file is not None:
            self.load_model(model_file)
        elif model_buffer is not None:
            self.load_model_buffer(model_buffer)

    def load_model(self, fname: str) -> None:
        check(self.lib, self.lib.XGBoosterLoadModel(self.handle, fname.encode()))

    def load_model_buffer(self, buf) -> None:
        if isinstance(buf, np.ndarray):
            ptr, n = buf.ctypes.data, buf.nbytes
            check(self.lib, self.lib.XGBoosterLoadModelFromBuffer(self.handle, ptr, n))
        else:
            b = bytes(buf)
            check(self.lib, self.lib.XGBoosterLoadModelFromBuffer(self.handle, C.cast(C.c_char_p(b), C.c_void_p), len(b)))

    def save_model(self, fname: str) -> None:
        check(self.lib, self.lib.XGBoosterSaveModel(self.handle, fname.encode()))

    def set_param(self, name: str, value) -> None:
        check(self.lib, self.lib.XGBoosterSetParam(self.handle, name.encode(), str(value).encode()))

    @property
    def num_groups(self) -> int:
        """Output groups of the loaded model (OHXBoosterGetNumGroups): max(num_class, num_target, 1)."""
        out = C.c_uint64()
        check(self.lib, self.lib.OHXBoosterGetNumGroups(self.handle, C.byref(out)))
        return int(out.value)

    def num_categorical_splits(self) -> int:
        """Nodes with a categorical split in the loaded model (OHXBoosterGetNumCategoricalSplits); 0 for a booster
        without one."""
        out = C.c_uint64()
        check(self.lib, self.lib.OHXBoosterGetNumCategoricalSplits(self.handle, C.byref(out)))
        return int(out.value)

    def _groups(self) -> int:
        # a library that only serves single-group boosters (the CPU oracle) has no OHXBoosterGetNumGroups
        return self.num_groups if hasattr(self.lib, "OHXBoosterGetNumGroups") else 1

    def predict(self, dmat: DMatrix, option_mask: int = 0, ntree_limit: int = 0, training: int = 0,
                copy: bool = True) -> np.ndarray:
        """Host result, float32: a copy of the booster-owned buffer, or (copy=False) a view of it that is valid until
        the booster's next predict - what the reference's Fortran reads through its c_f_pointer (OH_GridCompMod.F90:362).
        One output group: 1-D, as ever.  Several (num_groups >= 2): (nrow, G) margins or probabilities, (nrow, L) leaf
        ids in file tree order, and 1-D (nrow,) class indices for multi:softmax (include/ohxgb.h)."""
        n = C.c_uint64()
        ptr = C.POINTER(C.c_float)()
        check(self.lib, self.lib.XGBoosterPredict(self.handle, dmat.handle, option_mask, ntree_limit, training,
                                                   C.byref(n), C.byref(ptr)))
        if n.value == 0:
            return np.empty(0, dtype=np.float32)
        view = np.ctypeslib.as_array(ptr, shape=(n.value,))
        nrow = dmat.num_row
        if nrow and (n.value != nrow or option_mask == 16) and self._groups() >= 2:
            view = view.reshape(nrow, n.value // nrow)
        return view.copy() if copy else view

    def predict_device(self, dmat: DMatrix, out_ptr: int, option_mask: int = 0, ntree_limit: int = 0,
                       stream: int = 0) -> None:
        check(self.lib, self.lib.OHXBoosterPredictDevice(self.handle, dmat.handle, option_mask, ntree_limit, out_ptr,
                                                          stream))

    def check(self, stream: int = 0) -> None:
        check(self.lib, self.lib.OHXBoosterCheck(self.handle, stream))

    def predict_contribs(self, dmat: DMatrix, approximate: bool = False, ntree_limit: int = 0) -> np.ndarray:
        """Per-feature contributions, (nrow, F + 1) float32, column F the bias (OHXBoosterPredictContribs): exact
        TreeSHAP, or xgboost's approximate attribution with approximate=True.  Several output groups: (nrow, G, F + 1)."""
        n = C.c_uint64()
        ptr = C.POINTER(C.c_float)()
        check(self.lib, self.lib.OHXBoosterPredictContribs(self.handle, dmat.handle, int(bool(approximate)), ntree_limit,
                                                            C.byref(n), C.byref(ptr)))
        nrow = dmat.num_row
        if n.value == 0:
            return np.empty((nrow, 0), dtype=np.float32)
        G = self._groups()
        out = np.ctypeslib.as_array(ptr, shape=(n.value,)).reshape(nrow, n.value // nrow).copy()
        return out.reshape(nrow, G, n.value // nrow // G) if G >= 2 else out

    def predict_contribs_device(self, dmat: DMatrix, out_ptr: int, approximate: bool = False, ntree_limit: int = 0,
                                stream: int = 0) -> None:
        """The same into device memory: out_ptr holds nrow * (F + 1) float32; only enqueues on `stream`."""
        check(self.lib, self.lib.OHXBoosterPredictContribsDevice(self.handle, dmat.handle, int(bool(approximate)),
                                                                  ntree_limit, out_ptr, stream))

    def predict_interactions(self, dmat: DMatrix, approximate: bool = False, ntree_limit: int = 0) -> np.ndarray:
        """SHAP interaction values, (nrow, F + 1, F + 1) float32, index F the bias (OHXBoosterPredictInteractions):
        exact, or with approximate=True the approximate contributions on the diagonal.  Several output groups:
        (nrow, G, F + 1, F + 1)."""
        n = C.c_uint64()
        ptr = C.POINTER(C.c_float)()
        check(self.lib, self.lib.OHXBoosterPredictInteractions(self.handle, dmat.handle, int(bool(approximate)),
                                                                ntree_limit, C.byref(n), C.byref(ptr)))
        nrow = dmat.num_row
        if n.value == 0:
            return np.empty((nrow, 0, 0), dtype=np.float32)
        G = self._groups()
        side = int(round((n.value // nrow // G) ** 0.5))
        out = np.ctypeslib.as_array(ptr, shape=(n.value,))
        return (out.reshape(nrow, G, side, side) if G >= 2 else out.reshape(nrow, side, side)).copy()

    def predict_interactions_device(self, dmat: DMatrix, out_ptr: int, approximate: bool = False,
                                    ntree_limit: int = 0, stream: int = 0) -> None:
        """The same into device memory: out_ptr holds nrow * (F + 1)^2 float32; only enqueues on `stream`."""
        check(self.lib, self.lib.OHXBoosterPredictInteractionsDevice(self.handle, dmat.handle, int(bool(approximate)),
                                                                      ntree_limit, out_ptr, stream))

    def count_visits(self, dmat: DMatrix) -> None:
        """OHXBoosterCountVisits: every row of `dmat` walks every tree as a margin predict does and adds one to the
        counter of the leaf it reaches; counts accumulate until reset_visit_counts or a model load.  Returns when the
        rows are added."""
        check(self.lib, self.lib.OHXBoosterCountVisits(self.handle, dmat.handle))

    def count_visits_device(self, dmat: DMatrix, stream: int = 0) -> None:
        """The same, only enqueued on `stream` (not capturable)."""
        check(self.lib, self.lib.OHXBoosterCountVisitsDevice(self.handle, dmat.handle, stream or None))

    def visit_counts(self, stream: int = 0):
        """OHXBoosterGetVisitCounts -> (counts, rows_seen): counts[t][n] = the counted rows that passed node n of file
        tree t (np.uint64, file node numbering; copies).  Waits for `stream`."""
        ntree, seen = C.c_uint64(), C.c_uint64()
        offs, cnt = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        check(self.lib, self.lib.OHXBoosterGetVisitCounts(self.handle, stream or None, C.byref(ntree), C.byref(offs),
                                                           C.byref(cnt), C.byref(seen)))
        if ntree.value == 0:
            return [], int(seen.value)
        o = [int(offs[t]) for t in range(ntree.value + 1)]
        flat = np.ctypeslib.as_array(cnt, shape=(max(o[-1], 1),))
        return [flat[o[t]:o[t + 1]].astype(np.uint64) for t in range(ntree.value)], int(seen.value)

    def reset_visit_counts(self) -> None:
        check(self.lib, self.lib.OHXBoosterResetVisitCounts(self.handle))

    def refresh_cover(self, prior_weight: float = 0.0, stream: int = 0) -> None:
        """OHXBoosterRefreshCover: sum_hess := float32(count) + prior_weight * sum_hess for every reachable node, all or
        nothing; contributions computed afterwards are weighted by the counted data's covers."""
        check(self.lib, self.lib.OHXBoosterRefreshCover(self.handle, stream or None, prior_weight))

    REFIT_UNVISITED = {"keep": 0, "zero": 1}

    def refit_leaves(self, dmat: DMatrix, labels, eta: float = 1.0, reg_lambda: float = 1.0,
                     unvisited: str = "keep") -> int:
        """OHXBoosterRefitLeaves: every tree keeps its structure, every leaf value is estimated again from the rows of
        `dmat` and `labels` (squared error: w = -G / (H + reg_lambda), leaf = w * eta, tree after tree).  A leaf no row
        reaches keeps its value (unvisited="keep") or becomes 0 ("zero", as xgboost).  All or nothing; returns the
        number of leaves that were refit."""
        y = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
        n = C.c_uint64()
        check(self.lib, self.lib.OHXBoosterRefitLeaves(self.handle, dmat.handle, y.ctypes.data, y.size, eta, reg_lambda,
                                                        self.REFIT_UNVISITED[unvisited], C.byref(n)))
        return int(n.value)

    def refit_leaves_device(self, dmat: DMatrix, labels_ptr: int, nlabel: int, eta: float = 1.0,
                            reg_lambda: float = 1.0, unvisited: str = "keep", stream: int = 0) -> int:
        """The same with the labels in device memory (labels_ptr: a torch data_ptr() of nlabel float32, ready on
        `stream`); enqueues on `stream` and waits for it once at the end (not capturable)."""
        n = C.c_uint64()
        check(self.lib, self.lib.OHXBoosterRefitLeavesDevice(self.handle, dmat.handle, labels_ptr, nlabel, eta,
                                                              reg_lambda, self.REFIT_UNVISITED[unvisited], C.byref(n),
                                                              stream or None))
        return int(n.value)

    @staticmethod
    def _cuts(cuts):
        cut_ptr, cut_values = cuts
        cut_ptr = np.ascontiguousarray(cut_ptr, dtype=np.uint64).reshape(-1)
        cut_values = np.ascontiguousarray(cut_values, dtype=np.float32).reshape(-1)
        if cut_values.size == 0:
            cut_values = np.zeros(1, dtype=np.float32)      # (a pointer that is not NULL)
        return cut_ptr, cut_values

    def boost_trees(self, dmat: DMatrix, labels, cuts, rounds: int = 1, max_depth: int = 6, eta: float = 0.3,
                    reg_lambda: float = 1.0, gamma: float = 0.0, min_child_rows: int = 1) -> int:
        """OHXBoosterBoostTrees: `rounds` trees of depth <= max_depth are fitted on the GPU to the squared-error gradient
        of the rows of `dmat` and `labels`, from histograms over `cuts` = (cut_ptr, cut_values) (quantile_cuts makes
        them), and appended to the forest.  All or nothing; returns the number of nodes added."""
        y = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
        cut_ptr, cut_values = self._cuts(cuts)
        n = C.c_uint64()
        check(self.lib, self.lib.OHXBoosterBoostTrees(self.handle, dmat.handle, y.ctypes.data, y.size, cut_ptr.ctypes.data,
                                                       cut_values.ctypes.data, rounds, max_depth, eta, reg_lambda, gamma,
                                                       min_child_rows, C.byref(n)))
        return int(n.value)

    def boost_trees_device(self, dmat: DMatrix, labels_ptr: int, nlabel: int, cuts, rounds: int = 1, max_depth: int = 6,
                           eta: float = 0.3, reg_lambda: float = 1.0, gamma: float = 0.0, min_child_rows: int = 1,
                           stream: int = 0) -> int:
        """The same with the labels in device memory (labels_ptr: a torch data_ptr() of nlabel float32, ready on
        `stream`; the cuts stay host arrays); enqueues on `stream` and waits for it once at the end (not capturable)."""
        cut_ptr, cut_values = self._cuts(cuts)
        n = C.c_uint64()
        check(self.lib, self.lib.OHXBoosterBoostTreesDevice(self.handle, dmat.handle, labels_ptr, nlabel,
                                                             cut_ptr.ctypes.data, cut_values.ctypes.data, rounds,
                                                             max_depth, eta, reg_lambda, gamma, min_child_rows,
                                                             C.byref(n), stream or None))
        return int(n.value)

    @staticmethod
    def _eval_result(train, held, run, best, n, has_eval):
        k = int(run.value) + 1
        return {"train_rmse": train[:k].copy(), "eval_rmse": held[:k].copy() if has_eval else None,
                "rounds_run": int(run.value), "best_round": int(best.value), "nodes_added": int(n.value)}

    def boost_trees_eval(self, dmat: DMatrix, labels, cuts, eval_set=None, rounds: int = 1, max_depth: int = 6,
                         eta: float = 0.3, reg_lambda: float = 1.0, gamma: float = 0.0, min_child_rows: int = 1,
                         patience: int = 0) -> dict:
        """OHXBoosterBoostTreesEval: boost_trees with the RMSE of the training rows, and of the held-out
        eval_set = (DMatrix, labels) where one is given, after every round - computed on the GPU from exact integer
        sums.  patience >= 1 stops once the held-out error has not improved for that many rounds and keeps the trees up
        to the best round only.  -> dict: train_rmse and eval_rmse (float64, entries 0 .. rounds_run; eval_rmse None
        without an eval_set), rounds_run, best_round, nodes_added."""
        y = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
        cut_ptr, cut_values = self._cuts(cuts)
        ed, ey = (eval_set[0], np.ascontiguousarray(eval_set[1], dtype=np.float32).reshape(-1)) if eval_set is not None else (None, None)
        k = max(int(rounds), 0) + 1
        train, held = np.full(k, np.nan), np.full(k, np.nan)
        run, best, n = C.c_int32(), C.c_int32(), C.c_uint64()
        check(self.lib, self.lib.OHXBoosterBoostTreesEval(
            self.handle, dmat.handle, y.ctypes.data, y.size, ed.handle if ed is not None else None,
            ey.ctypes.data if ey is not None else None, ey.size if ey is not None else 0, cut_ptr.ctypes.data,
            cut_values.ctypes.data, rounds, max_depth, eta, reg_lambda, gamma, min_child_rows, patience,
            train.ctypes.data, held.ctypes.data, C.byref(run), C.byref(best), C.byref(n)))
        return self._eval_result(train, held, run, best, n, ed is not None)

    def boost_trees_eval_device(self, dmat: DMatrix, labels_ptr: int, nlabel: int, cuts, eval_set=None, rounds: int = 1,
                                max_depth: int = 6, eta: float = 0.3, reg_lambda: float = 1.0, gamma: float = 0.0,
                                min_child_rows: int = 1, patience: int = 0, stream: int = 0) -> dict:
        """The same with the labels in device memory: labels_ptr, and eval_set = (DMatrix, eval_labels_ptr,
        eval_nlabel), are torch data_ptr()s of float32 ready on `stream`; the cuts stay host arrays.  Enqueues on
        `stream`; waits once at the end, and with patience >= 1 once a round (not capturable)."""
        cut_ptr, cut_values = self._cuts(cuts)
        ed, eptr, en = eval_set if eval_set is not None else (None, None, 0)
        k = max(int(rounds), 0) + 1
        train, held = np.full(k, np.nan), np.full(k, np.nan)
        run, best, n = C.c_int32(), C.c_int32(), C.c_uint64()
        check(self.lib, self.lib.OHXBoosterBoostTreesEvalDevice(
            self.handle, dmat.handle, labels_ptr, nlabel, ed.handle if ed is not None else None, eptr or None, en,
            cut_ptr.ctypes.data, cut_values.ctypes.data, rounds, max_depth, eta, reg_lambda, gamma, min_child_rows,
            patience, train.ctypes.data, held.ctypes.data, C.byref(run), C.byref(best), C.byref(n), stream or None))
        return self._eval_result(train, held, run, best, n, ed is not None)

    def _set_objective(self, objective, huber_slope, quantile_alpha=None, reg_alpha=None, max_delta_step=None, eval_metric=None,
                       monotone_constraints=None, colsample_bylevel=None, colsample_bynode=None, interaction_constraints=None) -> None:
        """objective= and huber_slope= of the boost_trees_* methods: "squarederror", "pseudohuber" and its slope, or
        "quantile", set on the handle by set_param("ohx_objective") and set_param("ohx_huber_slope") and kept for later
        calls (they go into no model file).  quantile_alpha= is alpha of the quantile objective and metric, set by
        "ohx_quantile_alpha"; the calls that refuse the quantile objective surface the refusal.
        reg_alpha=, max_delta_step= and eval_metric= ("rmse", "mae", "pseudohuber" or "quantile": what the two
        metric arrays hold and the stop rule compares) likewise, by "ohx_reg_alpha", "ohx_max_delta_step" and
        "ohx_eval_metric".  monotone_constraints= is a sequence of ints in {-1, 0, 1}, one a feature from feature 0 on, or
        the string itself ("(1,0,-1)"), set by "ohx_monotone_constraints"; () is none.  colsample_bylevel= and
        colsample_bynode= (the calls that carry a seed take them) are fractions in (0, 1], set by "ohx_colsample_bylevel" and
        "ohx_colsample_bynode".  interaction_constraints= is a list of lists of feature ids, the groups of features that may
        act together in one tree, or the string itself ("[[0, 2], [1, 3, 4]]"), set by "ohx_interaction_constraints"; [] is
        none.  None leaves the handle's setting."""
        if interaction_constraints is not None:
            if not isinstance(interaction_constraints, str):
                interaction_constraints = "[" + ",".join("[" + ",".join(str(int(f)) for f in g) + "]" for g in interaction_constraints) + "]"
            self.set_param("ohx_interaction_constraints", interaction_constraints)
        if colsample_bylevel is not None:
            self.set_param("ohx_colsample_bylevel", repr(float(colsample_bylevel)))
        if colsample_bynode is not None:
            self.set_param("ohx_colsample_bynode", repr(float(colsample_bynode)))
        if monotone_constraints is not None:
            if not isinstance(monotone_constraints, str):
                monotone_constraints = "(" + ",".join(str(int(c)) for c in monotone_constraints) + ")"
            self.set_param("ohx_monotone_constraints", monotone_constraints)
        if reg_alpha is not None:
            self.set_param("ohx_reg_alpha", repr(float(reg_alpha)))
        if max_delta_step is not None:
            self.set_param("ohx_max_delta_step", repr(float(max_delta_step)))
        if eval_metric is not None:
            self.set_param("ohx_eval_metric", eval_metric)
        if objective is not None:
            self.set_param("ohx_objective", objective)
        if huber_slope is not None:
            self.set_param("ohx_huber_slope", repr(float(huber_slope)))
        if quantile_alpha is not None:
            self.set_param("ohx_quantile_alpha", repr(float(quantile_alpha)))

    def boost_trees_weighted(self, dmat: DMatrix, labels, cuts, weights=None, eval_set=None, rounds: int = 1,
                             max_depth: int = 6, eta: float = 0.3, reg_lambda: float = 1.0, gamma: float = 0.0,
                             min_child_weight: float = 1.0, patience: int = 0,
                             *, objective=None, huber_slope=None, quantile_alpha=None, reg_alpha=None, max_delta_step=None,
                             eval_metric=None, monotone_constraints=None, interaction_constraints=None) -> dict:
        """OHXBoosterBoostTreesWeighted: boost_trees_eval with a weight per row (0 <= w < 256; None: all 1) in the
        histograms, the leaves and both RMSEs.  eval_set = (DMatrix, labels[, weights]).  min_child_weight stands where
        min_child_rows stood.  -> the dict of boost_trees_eval."""
        self._set_objective(objective, huber_slope, quantile_alpha, reg_alpha, max_delta_step, eval_metric, monotone_constraints,
                            interaction_constraints=interaction_constraints)
        return self._boost_weighted("OHXBoosterBoostTreesWeighted", dmat, labels, cuts, weights, eval_set, rounds, max_depth,
                                    eta, reg_lambda, gamma, min_child_weight, patience)

    def _boost_weighted(self, entry, dmat, labels, cuts, weights, eval_set, rounds, max_depth, eta, reg_lambda, gamma,
                        min_child_weight, patience) -> dict:
        """The host form of the Weighted call, or of an entry point with its argument list."""
        y = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1) if weights is not None else None
        if w is not None and w.size != y.size:
            raise ValueError(f"{w.size} weights for {y.size} labels")
        cut_ptr, cut_values = self._cuts(cuts)
        ed = ey = ew = None
        if eval_set is not None:
            ed, ey = eval_set[0], np.ascontiguousarray(eval_set[1], dtype=np.float32).reshape(-1)
            if len(eval_set) > 2 and eval_set[2] is not None:
                ew = np.ascontiguousarray(eval_set[2], dtype=np.float32).reshape(-1)
                if ew.size != ey.size:
                    raise ValueError(f"{ew.size} eval weights for {ey.size} eval labels")
        k = max(int(rounds), 0) + 1
        train, held = np.full(k, np.nan), np.full(k, np.nan)
        run, best, n = C.c_int32(), C.c_int32(), C.c_uint64()
        check(self.lib, getattr(self.lib, entry)(
            self.handle, dmat.handle, y.ctypes.data, w.ctypes.data if w is not None else None, y.size,
            ed.handle if ed is not None else None, ey.ctypes.data if ey is not None else None,
            ew.ctypes.data if ew is not None else None, ey.size if ey is not None else 0, cut_ptr.ctypes.data,
            cut_values.ctypes.data, rounds, max_depth, eta, reg_lambda, gamma, min_child_weight, patience,
            train.ctypes.data, held.ctypes.data, C.byref(run), C.byref(best), C.byref(n)))
        return self._eval_result(train, held, run, best, n, ed is not None)

    def boost_trees_weighted_device(self, dmat: DMatrix, labels_ptr: int, nlabel: int, cuts, weights_ptr: int = 0,
                                    eval_set=None, rounds: int = 1, max_depth: int = 6, eta: float = 0.3,
                                    reg_lambda: float = 1.0, gamma: float = 0.0, min_child_weight: float = 1.0,
                                    patience: int = 0, stream: int = 0,
                                    *, objective=None, huber_slope=None, quantile_alpha=None, reg_alpha=None, max_delta_step=None,
                             eval_metric=None, monotone_constraints=None, interaction_constraints=None) -> dict:
        """The same with labels and weights in device memory: labels_ptr, weights_ptr (0: all 1) and
        eval_set = (DMatrix, eval_labels_ptr, eval_nlabel[, eval_weights_ptr]) are torch data_ptr()s of float32 ready
        on `stream`; the cuts stay host arrays.  Enqueues on `stream`; waits as boost_trees_eval_device (not capturable)."""
        self._set_objective(objective, huber_slope, quantile_alpha, reg_alpha, max_delta_step, eval_metric, monotone_constraints,
                            interaction_constraints=interaction_constraints)
        return self._boost_weighted_device("OHXBoosterBoostTreesWeightedDevice", dmat, labels_ptr, nlabel, cuts, weights_ptr,
                                           eval_set, rounds, max_depth, eta, reg_lambda, gamma, min_child_weight, patience,
                                           stream)

    def _boost_weighted_device(self, entry, dmat, labels_ptr, nlabel, cuts, weights_ptr, eval_set, rounds, max_depth, eta,
                               reg_lambda, gamma, min_child_weight, patience, stream) -> dict:
        """The device form of the Weighted call, or of an entry point with its argument list."""
        cut_ptr, cut_values = self._cuts(cuts)
        ed, eptr, en, ewptr = (tuple(eval_set) + (0,))[:4] if eval_set is not None else (None, None, 0, 0)
        k = max(int(rounds), 0) + 1
        train, held = np.full(k, np.nan), np.full(k, np.nan)
        run, best, n = C.c_int32(), C.c_int32(), C.c_uint64()
        check(self.lib, getattr(self.lib, entry)(
            self.handle, dmat.handle, labels_ptr, weights_ptr or None, nlabel, ed.handle if ed is not None else None,
            eptr or None, ewptr or None, en, cut_ptr.ctypes.data, cut_values.ctypes.data, rounds, max_depth, eta,
            reg_lambda, gamma, min_child_weight, patience, train.ctypes.data, held.ctypes.data, C.byref(run),
            C.byref(best), C.byref(n), stream or None))
        return self._eval_result(train, held, run, best, n, ed is not None)

    def boost_trees_deep(self, dmat: DMatrix, labels, cuts, weights=None, eval_set=None, rounds: int = 1,
                         max_depth: int = 12, eta: float = 0.3, reg_lambda: float = 1.0, gamma: float = 0.0,
                         min_child_weight: float = 1.0, patience: int = 0,
                         *, objective=None, huber_slope=None, quantile_alpha=None, reg_alpha=None, max_delta_step=None,
                             eval_metric=None, monotone_constraints=None, interaction_constraints=None) -> dict:
        """OHXBoosterBoostTreesDeep: boost_trees_weighted with max_depth up to 18.  From level 8 on a level's histograms
        are kept in HBM for a batch of nodes at a time, and the call waits once a level for the ids of the open nodes.
        Up to depth 8 it is boost_trees_weighted itself.  -> the dict of boost_trees_eval."""
        self._set_objective(objective, huber_slope, quantile_alpha, reg_alpha, max_delta_step, eval_metric, monotone_constraints,
                            interaction_constraints=interaction_constraints)
        return self._boost_weighted("OHXBoosterBoostTreesDeep", dmat, labels, cuts, weights, eval_set, rounds, max_depth, eta,
                                    reg_lambda, gamma, min_child_weight, patience)

    def boost_trees_deep_device(self, dmat: DMatrix, labels_ptr: int, nlabel: int, cuts, weights_ptr: int = 0,
                                eval_set=None, rounds: int = 1, max_depth: int = 12, eta: float = 0.3,
                                reg_lambda: float = 1.0, gamma: float = 0.0, min_child_weight: float = 1.0,
                                patience: int = 0, stream: int = 0,
                                *, objective=None, huber_slope=None, quantile_alpha=None, reg_alpha=None, max_delta_step=None,
                             eval_metric=None, monotone_constraints=None, interaction_constraints=None) -> dict:
        """The same with labels and weights in device memory, as boost_trees_weighted_device takes them.  With
        max_depth > 8 the call waits for `stream` once a level from level 7 on."""
        self._set_objective(objective, huber_slope, quantile_alpha, reg_alpha, max_delta_step, eval_metric, monotone_constraints,
                            interaction_constraints=interaction_constraints)
        return self._boost_weighted_device("OHXBoosterBoostTreesDeepDevice", dmat, labels_ptr, nlabel, cuts, weights_ptr,
                                           eval_set, rounds, max_depth, eta, reg_lambda, gamma, min_child_weight, patience,
                                           stream)

    def boost_trees_sampled(self, dmat: DMatrix, labels, cuts, weights=None, eval_set=None, rounds: int = 1,
                            max_depth: int = 6, eta: float = 0.3, reg_lambda: float = 1.0, gamma: float = 0.0,
                            min_child_weight: float = 1.0, subsample: float = 1.0, colsample_bytree: float = 1.0,
                            seed: int = 0, patience: int = 0,
                            *, objective=None, huber_slope=None, quantile_alpha=None, reg_alpha=None, max_delta_step=None,
                             eval_metric=None, monotone_constraints=None, colsample_bylevel=None, colsample_bynode=None,
                             interaction_constraints=None) -> dict:
        """OHXBoosterBoostTreesSampled: boost_trees_weighted where every tree is fitted to a fresh bag of the rows
        (a fraction `subsample`) and may split on a fresh set of the features (a fraction `colsample_bytree`), both
        drawn on the GPU from `seed` (a uint64) and the tree's index in the forest.  colsample_bylevel= and
        colsample_bynode= narrow the tree's features again for every level and every node.  -> the dict of boost_trees_eval."""
        self._set_objective(objective, huber_slope, quantile_alpha, reg_alpha, max_delta_step, eval_metric, monotone_constraints,
                            colsample_bylevel, colsample_bynode, interaction_constraints=interaction_constraints)
        return self._boost_sampled("OHXBoosterBoostTreesSampled", dmat, labels, cuts, weights, eval_set, rounds, max_depth, eta,
                                   reg_lambda, gamma, min_child_weight, subsample, colsample_bytree, seed, patience)

    def _boost_sampled(self, entry, dmat, labels, cuts, weights, eval_set, rounds, max_depth, eta, reg_lambda, gamma,
                       min_child_weight, subsample, colsample_bytree, seed, patience) -> dict:
        """The host form of the Sampled call, or of an entry point with its argument list."""
        y = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1) if weights is not None else None
        if w is not None and w.size != y.size:
            raise ValueError(f"{w.size} weights for {y.size} labels")
        cut_ptr, cut_values = self._cuts(cuts)
        ed = ey = ew = None
        if eval_set is not None:
            ed, ey = eval_set[0], np.ascontiguousarray(eval_set[1], dtype=np.float32).reshape(-1)
            if len(eval_set) > 2 and eval_set[2] is not None:
                ew = np.ascontiguousarray(eval_set[2], dtype=np.float32).reshape(-1)
                if ew.size != ey.size:
                    raise ValueError(f"{ew.size} eval weights for {ey.size} eval labels")
        k = max(int(rounds), 0) + 1
        train, held = np.full(k, np.nan), np.full(k, np.nan)
        run, best, n = C.c_int32(), C.c_int32(), C.c_uint64()
        check(self.lib, getattr(self.lib, entry)(
            self.handle, dmat.handle, y.ctypes.data, w.ctypes.data if w is not None else None, y.size,
            ed.handle if ed is not None else None, ey.ctypes.data if ey is not None else None,
            ew.ctypes.data if ew is not None else None, ey.size if ey is not None else 0, cut_ptr.ctypes.data,
            cut_values.ctypes.data, rounds, max_depth, eta, reg_lambda, gamma, min_child_weight, subsample,
            colsample_bytree, int(seed) & 0xFFFFFFFFFFFFFFFF, patience, train.ctypes.data, held.ctypes.data, C.byref(run),
            C.byref(best), C.byref(n)))
        return self._eval_result(train, held, run, best, n, ed is not None)

    def boost_trees_sampled_device(self, dmat: DMatrix, labels_ptr: int, nlabel: int, cuts, weights_ptr: int = 0,
                                   eval_set=None, rounds: int = 1, max_depth: int = 6, eta: float = 0.3,
                                   reg_lambda: float = 1.0, gamma: float = 0.0, min_child_weight: float = 1.0,
                                   subsample: float = 1.0, colsample_bytree: float = 1.0, seed: int = 0,
                                   patience: int = 0, stream: int = 0,
                                   *, objective=None, huber_slope=None, quantile_alpha=None, reg_alpha=None, max_delta_step=None,
                             eval_metric=None, monotone_constraints=None, colsample_bylevel=None, colsample_bynode=None,
                             interaction_constraints=None) -> dict:
        """The same with labels and weights in device memory, as boost_trees_weighted_device takes them."""
        self._set_objective(objective, huber_slope, quantile_alpha, reg_alpha, max_delta_step, eval_metric, monotone_constraints,
                            colsample_bylevel, colsample_bynode, interaction_constraints=interaction_constraints)
        return self._boost_sampled_device("OHXBoosterBoostTreesSampledDevice", dmat, labels_ptr, nlabel, cuts, weights_ptr,
                                          eval_set, rounds, max_depth, eta, reg_lambda, gamma, min_child_weight, subsample,
                                          colsample_bytree, seed, patience, stream)

    def _boost_sampled_device(self, entry, dmat, labels_ptr, nlabel, cuts, weights_ptr, eval_set, rounds, max_depth, eta,
                              reg_lambda, gamma, min_child_weight, subsample, colsample_bytree, seed, patience, stream) -> dict:
        """The device form of the Sampled call, or of an entry point with its argument list."""
        cut_ptr, cut_values = self._cuts(cuts)
        ed, eptr, en, ewptr = (tuple(eval_set) + (0,))[:4] if eval_set is not None else (None, None, 0, 0)
        k = max(int(rounds), 0) + 1
        train, held = np.full(k, np.nan), np.full(k, np.nan)
        run, best, n = C.c_int32(), C.c_int32(), C.c_uint64()
        check(self.lib, getattr(self.lib, entry)(
            self.handle, dmat.handle, labels_ptr, weights_ptr or None, nlabel, ed.handle if ed is not None else None,
            eptr or None, ewptr or None, en, cut_ptr.ctypes.data, cut_values.ctypes.data, rounds, max_depth, eta,
            reg_lambda, gamma, min_child_weight, subsample, colsample_bytree, int(seed) & 0xFFFFFFFFFFFFFFFF, patience,
            train.ctypes.data, held.ctypes.data, C.byref(run), C.byref(best), C.byref(n), stream or None))
        return self._eval_result(train, held, run, best, n, ed is not None)

    def boost_trees_deep_sampled(self, dmat: DMatrix, labels, cuts, weights=None, eval_set=None, rounds: int = 1,
                                 max_depth: int = 12, eta: float = 0.3, reg_lambda: float = 1.0, gamma: float = 0.0,
                                 min_child_weight: float = 1.0, subsample: float = 1.0, colsample_bytree: float = 1.0,
                                 seed: int = 0, patience: int = 0,
                                 *, objective=None, huber_slope=None, quantile_alpha=None, reg_alpha=None, max_delta_step=None,
                             eval_metric=None, monotone_constraints=None, colsample_bylevel=None, colsample_bynode=None,
                             interaction_constraints=None) -> dict:
        """OHXBoosterBoostTreesDeepSampled: boost_trees_sampled with max_depth up to 18.  From level 8 on a level's
        histograms are kept in HBM for a batch of nodes at a time, over the bag's rows and the tree's features only, and
        the call waits once a level for the ids of the open nodes.  Up to depth 8 it is boost_trees_sampled itself; with
        both fractions 1 it is boost_trees_deep.  -> the dict of boost_trees_eval."""
        self._set_objective(objective, huber_slope, quantile_alpha, reg_alpha, max_delta_step, eval_metric, monotone_constraints,
                            colsample_bylevel, colsample_bynode, interaction_constraints=interaction_constraints)
        return self._boost_sampled("OHXBoosterBoostTreesDeepSampled", dmat, labels, cuts, weights, eval_set, rounds, max_depth,
                                   eta, reg_lambda, gamma, min_child_weight, subsample, colsample_bytree, seed, patience)

    def boost_trees_deep_sampled_device(self, dmat: DMatrix, labels_ptr: int, nlabel: int, cuts, weights_ptr: int = 0,
                                        eval_set=None, rounds: int = 1, max_depth: int = 12, eta: float = 0.3,
                                        reg_lambda: float = 1.0, gamma: float = 0.0, min_child_weight: float = 1.0,
                                        subsample: float = 1.0, colsample_bytree: float = 1.0, seed: int = 0,
                                        patience: int = 0, stream: int = 0,
                                        *, objective=None, huber_slope=None, quantile_alpha=None, reg_alpha=None, max_delta_step=None,
                             eval_metric=None, monotone_constraints=None, colsample_bylevel=None, colsample_bynode=None,
                             interaction_constraints=None) -> dict:
        """The same with labels and weights in device memory, as boost_trees_weighted_device takes them.  With
        max_depth > 8 the call waits for `stream` once a level from level 7 on."""
        self._set_objective(objective, huber_slope, quantile_alpha, reg_alpha, max_delta_step, eval_metric, monotone_constraints,
                            colsample_bylevel, colsample_bynode, interaction_constraints=interaction_constraints)
        return self._boost_sampled_device("OHXBoosterBoostTreesDeepSampledDevice", dmat, labels_ptr, nlabel, cuts, weights_ptr,
                                          eval_set, rounds, max_depth, eta, reg_lambda, gamma, min_child_weight, subsample,
                                          colsample_bytree, seed, patience, stream)

    def predict_fields(self, fields: Sequence[np.ndarray], is2d: Sequence[bool], pl_feature: int, im: int, jm: int,
                       km: int, k1: int, k2: int, missing: float, oh_ml: np.ndarray, *, apply_pow10: bool = True,
                       ohscale: float = 1.0, margin: Optional[np.ndarray] = None) -> None:
        """Host arrays in Fortran order (pass the .T views' buffers: index i + im*(j + jm*k))."""
        nf = len(fields)
        ptrs = (C.c_void_p * nf)(*[f.ctypes.data for f in fields])
        flags = (C.c_int32 * nf)(*[1 if b else 0 for b in is2d])
        check(self.lib, self.lib.OHXBoosterPredictFields(
            self.handle, ptrs, flags, nf, pl_feature, im, jm, km, k1, k2, missing, 1 if apply_pow10 else 0, ohscale,
            oh_ml.ctypes.data, margin.ctypes.data if margin is not None else None))

    def predict_fields_device(self, field_ptrs: Sequence[int], is2d: Sequence[bool], pl_feature: int, im: int,
                              jm: int, km: int, k1: int, k2: int, missing: float, oh_ml_ptr: int, *,
                              apply_pow10: bool = True, ohscale: float = 1.0, margin_ptr: int = 0,
                              stream: int = 0) -> None:
        nf = len(field_ptrs)
        ptrs = (C.c_void_p * nf)(*field_ptrs)
        flags = (C.c_int32 * nf)(*[1 if b else 0 for b in is2d])
        check(self.lib, self.lib.OHXBoosterPredictFieldsDevice(
            self.handle, ptrs, flags, nf, pl_feature, im, jm, km, k1, k2, missing, 1 if apply_pow10 else 0, ohscale,
            oh_ml_ptr, margin_ptr or None, stream or None))

    def predict_contribs_fields(self, fields: Sequence[np.ndarray], is2d: Sequence[bool], pl_feature: int, im: int,
                                jm: int, km: int, k1: int, k2: int, missing: float,
                                out: Sequence[Optional[np.ndarray]], *, approximate: bool = False,
                                ntree_limit: int = 0) -> None:
        """Per-feature contributions of the slab k1..k2 (1-based) from the fields, as predict_fields gathers them
        (OHXBoosterPredictContribsFields).  `out` holds F + 1 entries, F the booster's feature count: writable
        Fortran-order float32 host arrays of im * jm * km elements (out[F] the bias), or None for one not wanted."""
        nf = len(fields)
        for a in out:
            if a is not None and (not isinstance(a, np.ndarray) or a.dtype != np.float32 or
                                  not a.flags["F_CONTIGUOUS"] or not a.flags["WRITEABLE"] or a.size < im * jm * km):
                raise ValueError("out: writable Fortran-order float32 arrays of at least im * jm * km elements, or None")
        ptrs = (C.c_void_p * nf)(*[f.ctypes.data for f in fields])
        flags = (C.c_int32 * nf)(*[1 if b else 0 for b in is2d])
        # padded with NULLs to the most entries the library reads (F + 1, F <= 32 for the fields forms)
        outs = (C.c_void_p * max(len(out), 33))(*[a.ctypes.data if a is not None else None for a in out])
        check(self.lib, self.lib.OHXBoosterPredictContribsFields(
            self.handle, ptrs, flags, nf, pl_feature, im, jm, km, k1, k2, missing, int(bool(approximate)), ntree_limit,
            outs))

    def predict_contribs_fields_device(self, field_ptrs: Sequence[int], is2d: Sequence[bool], pl_feature: int,
                                       im: int, jm: int, km: int, k1: int, k2: int, missing: float,
                                       out_ptrs: Sequence[int], *, approximate: bool = False, ntree_limit: int = 0,
                                       stream: int = 0) -> None:
        """The same on device pointers (out_ptrs: F + 1 device addresses, 0 for one not wanted); only enqueues on
        `stream`."""
        nf = len(field_ptrs)
        ptrs = (C.c_void_p * nf)(*field_ptrs)
        flags = (C.c_int32 * nf)(*[1 if b else 0 for b in is2d])
        outs = (C.c_void_p * max(len(out_ptrs), 33))(*[p or None for p in out_ptrs])
        check(self.lib, self.lib.OHXBoosterPredictContribsFieldsDevice(
            self.handle, ptrs, flags, nf, pl_feature, im, jm, km, k1, k2, missing, int(bool(approximate)), ntree_limit,
            outs, stream or None))

    def explain_cells(self, fields, is2d: Sequence[bool], pl_feature: int, im: int, jm: int, km: int, missing: float, *,
                      box=None, a=None, b=None, b0: float = 0.0, cells=None, what: str = "contribs",
                      approximate: bool = False, ntree_limit: int = 0, scatter: bool = True,
                      fill: float = float("nan")):
        """Contributions (what="contribs") or SHAP interaction values (what="interactions") of selected gridcells,
        from device fields, on torch's current stream: select_cells_device (unless `cells`, an int64 device tensor, is
        given) -> gather_cells_device -> OHXDMatrixCreateFromDevice -> OHXBoosterPredictContribsDevice / ...InteractionsDevice
        -> scatter_cells_device, one call per output column.  `fields`, `a`, `b`: torch float32 device tensors, a field
        (im,jm,km) or (im,jm) in Fortran order; `a` / `b` count as 2-D when they hold im * jm elements.  Waits once,
        for the count of the selection.  Returns (cells, out): `out` a (columns, im*jm*km) tensor, row c the
        Fortran-order array of output column c (F + 1 columns, (F + 1)^2 for interactions, times the booster's
        groups), `fill` where no cell was selected; with scatter=False the per-cell tensor (ncell, columns)."""
        import torch
        if what not in ("contribs", "interactions"):
            raise ValueError("what: 'contribs' or 'interactions'")
        dev = fields[0].device
        stream = torch.cuda.current_stream(dev).cuda_stream
        total = im * jm * km
        if cells is None:
            i1, i2, j1, j2, k1, k2 = box or (1, im, 1, jm, 1, km)
            cap = max(0, (i2 - i1 + 1) * (j2 - j1 + 1) * (k2 - k1 + 1))
            cells = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            select_cells_device(im, jm, km, (i1, i2, j1, j2, k1, k2), a.data_ptr() if a is not None else 0,
                                a is not None and a.numel() == im * jm, b.data_ptr() if b is not None else 0,
                                b is not None and b.numel() == im * jm, b0, cells.data_ptr(), cap, count.data_ptr(),
                                stream=stream, lib=self.lib)
            cells = cells[:int(count.item())]
        ncell = int(cells.numel())
        nf = len(fields)
        F = self.info()["num_feature"]
        ncol = self._groups() * ((F + 1) if what == "contribs" else (F + 1) * (F + 1))
        rows = torch.empty((max(ncell, 1), nf), dtype=torch.float32, device=dev)
        vals = torch.empty((max(ncell, 1), ncol), dtype=torch.float32, device=dev)
        gather_cells_device([f.data_ptr() for f in fields], is2d, pl_feature, im, jm, km, cells.data_ptr(), ncell,
                            rows.data_ptr(), stream=stream, lib=self.lib)
        if ncell:
            dmat = DMatrix(device_ptr=rows.data_ptr(), nrow=ncell, ncol=nf, missing=missing, lib=self.lib)
            try:
                if what == "contribs":
                    self.predict_contribs_device(dmat, vals.data_ptr(), approximate, ntree_limit, stream)
                else:
                    self.predict_interactions_device(dmat, vals.data_ptr(), approximate, ntree_limit, stream)
            finally:
                dmat.free()
        if not scatter:
            return cells, vals[:ncell]
        out = torch.full((ncol, total), fill, dtype=torch.float32, device=dev)
        for c in range(ncol):
            scatter_cells_device(vals.data_ptr(), ncol, c, cells.data_ptr(), ncell, out[c].data_ptr(), im, jm, km,
                                 stream=stream, lib=self.lib)
        return cells, out

    def run1_prepare(self, state: dict, *, dynamic_k_range: bool, tropp_min: float = 4000.0, ohscale: float = 0.85,
                     missing: float = -999.0, avogad: float = 6.023e26, runiv: float = 8314.47,
                     epsilon: float = 18.015 / 28.965, want_boost: bool = True, want_ndwet: bool = True,
                     want_diag: bool = False) -> dict:
        """The OHXRun1Args of a tick, built once: `state` maps the names of OHXRun1Args to [i,j(,k)]-indexed float32
        arrays (edge fields have km+1 levels; "scacoef" is a list of seven).  The returned call keeps the flattened
        host arrays alive at fixed addresses - as MAPL's state pointers are from tick to tick - so that run1_call can
        be repeated on them (and ohx_register_host has something stable to register)."""
        def flat(a):
            return np.ascontiguousarray(np.asarray(a, dtype=np.float32).T)
        im, jm, km = state["t_mod"].shape
        keep = {}
        args = OHXRun1Args()
        args.im, args.jm, args.km = im, jm, km
        args.dynamic_k_range = 1 if dynamic_k_range else 0
        args.tropp_min, args.ohscale, args.missing = tropp_min, ohscale, missing
        args.avogad, args.runiv, args.epsilon = avogad, runiv, epsilon
        for name in RUN1_INPUTS_3D + RUN1_INPUTS_EDGE + RUN1_INPUTS_2D:
            keep[name] = flat(state[name])
            setattr(args, name, keep[name].ctypes.data)
        sca = [flat(a) for a in state["scacoef"]]
        keep["sca"] = sca
        args.scacoef = (C.c_void_p * 7)(*[a.ctypes.data for a in sca])
        oh = np.zeros(im * jm * km, dtype=np.float32)
        boost = np.zeros(im * jm * km, dtype=np.float32) if want_boost else None
        ndwet = np.zeros(im * jm * km, dtype=np.float32) if want_ndwet else None
        k1, k2 = C.c_int32(), C.c_int32()
        args.oh = oh.ctypes.data
        args.oh_boost = boost.ctypes.data if want_boost else None
        args.ndwet = ndwet.ctypes.data if want_ndwet else None
        args.k1 = C.cast(C.pointer(k1), C.c_void_p)
        args.k2 = C.cast(C.pointer(k2), C.c_void_p)
        diag = {}
        if want_diag:
            for name in RUN1_DIAG_3D:
                diag[name] = np.zeros(im * jm * km, dtype=np.float32)
                setattr(args, name, diag[name].ctypes.data)
            diag["diag_strato3"] = np.zeros(im * jm, dtype=np.float32)
            args.diag_strato3 = diag["diag_strato3"].ctypes.data
        return {"args": args, "keep": keep, "oh": oh, "boost": boost, "ndwet": ndwet, "k1": k1, "k2": k2, "diag": diag,
                "shape": (im, jm, km)}

    def run1_call(self, call: dict) -> dict:
        """OHXBoosterRun1 on the host arrays of a prepared call.  Returns {"oh", "oh_boost", "ndwet", "k1", "k2"} (+ the
        DIAG dumps) as views of the call's output arrays, indexed [i,j,k]."""
        im, jm, km = call["shape"]
        check(self.lib, self.lib.OHXBoosterRun1(self.handle, C.byref(call["args"])))
        unflat = lambda a: None if a is None else a.reshape(km, jm, im).transpose(2, 1, 0)   # noqa: E731
        out = {"oh": unflat(call["oh"]), "oh_boost": unflat(call["boost"]), "ndwet": unflat(call["ndwet"]),
               "k1": call["k1"].value, "k2": call["k2"].value}
        for name, a in call["diag"].items():
            out[name] = a.reshape(jm, im).T if name == "diag_strato3" else unflat(a)
        return out

    def run1(self, state: dict, **kw) -> dict:
        """OHXBoosterRun1 on host arrays (run1_prepare + run1_call)."""
        return self.run1_call(self.run1_prepare(state, **kw))

    def info(self) -> dict:
        arr = (C.c_uint64 * 8)()
        check(self.lib, self.lib.OHXBoosterGetInfo(self.handle, arr))
        keys = ["num_trees", "num_nodes", "num_slots", "node_bytes", "max_depth", "num_feature", "packed",
                "gathers_per_wave"]
        return {k: int(arr[i]) for i, k in enumerate(keys)}

    def ring_reruns(self, stream: int = 0) -> int:
        """How often a ring block gave up and the tile kernel predicted the batch again (include/ohxgb.h)."""
        out = C.c_uint64()
        check(self.lib, self.lib.OHXBoosterRingReruns(self.handle, stream, C.byref(out)))
        return int(out.value)

    def copy_engine_choice(self):
        """-> (choice, trials, picked_dma): what ohx_copy_engine = auto decided for this booster's Run1 host form
        (-1 trying / not in charge, 0 copy kernels, 1 DMA), and how its trials went (include/ohxgb.h)."""
        c, t, d = C.c_int(), C.c_uint(), C.c_uint()
        check(self.lib, self.lib.OHXBoosterCopyEngineChoice(self.handle, C.byref(c), C.byref(t), C.byref(d)))
        return int(c.value), int(t.value), int(d.value)

    def kernel_symbol(self, ncol: int) -> str:
        out = C.c_char_p()
        check(self.lib, self.lib.OHXBoosterKernelSymbol(self.handle, ncol, C.byref(out)))
        return out.value.decode()

    def kernel_symbols_for(self, dmat) -> str:
        """Every kernel a margin predict on `dmat` launches, in order, joined by " + " (OHXBoosterKernelSymbolRows)."""
        out = C.c_char_p()
        check(self.lib, self.lib.OHXBoosterKernelSymbolRows(self.handle, dmat.handle, C.byref(out)))
        return out.value.decode()

    def fields_kernel_symbol(self, nrow: int = 1 << 30) -> str:
        """The __global__ the fused OHXBoosterPredictFields launches for a slab of `nrow` gridcells: the fields kernel of
        the same family as the rows kernel (kernels.hip launch_predict_fields; the ring kernel from two residencies
        of the chip on)."""
        import re
        rows = self.kernel_symbol(27)
        if "ring" in rows:
            return "predict_fields_ring_kernel" if nrow >= 256 * 16 * 64 * 2 else "predict_fields_kernel<2,2,true>"
        m = re.match(r"predict_rows_tile_kernel<(\d+),(\d+),(?:true|false),(true|false)>", rows)
        return f"predict_fields_kernel<{m.group(1)},{m.group(2)},{m.group(3)}>" if m else "predict_fields_kernel<0,1,false>"

    def free(self) -> None:
        if self.handle:
            check(self.lib, self.lib.XGBoosterFree(self.handle))
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def oh_post_process(ple_mod, t_mod, q_mod, tropp_mod, default_oh, oh_ml, *, avogad: float = 6.023e26,
                    runiv: float = 8314.47, epsilon: float = 18.015 / 28.965, lib: Optional[C.CDLL] = None):
    """OHXOHPostProcess on [i,j(,k)]-indexed float32 arrays -> (oh, ndwet), indexed [i,j,k]."""
    lib = lib or load_library()
    if not hasattr(lib.OHXOHPostProcess, "argtypes") or lib.OHXOHPostProcess.argtypes is None:
        lib.OHXOHPostProcess.argtypes = [C.c_int] * 3 + [C.c_float] * 3 + [C.c_void_p] * 8
    flat = [np.ascontiguousarray(np.asarray(a, dtype=np.float32).T) for a in (ple_mod, t_mod, q_mod, tropp_mod, default_oh, oh_ml)]
    im, jm, km = np.asarray(t_mod).shape
    oh = np.zeros(im * jm * km, dtype=np.float32)
    ndwet = np.zeros(im * jm * km, dtype=np.float32)
    check(lib, lib.OHXOHPostProcess(im, jm, km, avogad, runiv, epsilon, *[a.ctypes.data for a in flat], oh.ctypes.data,
                                    ndwet.ctypes.data))
    return oh.reshape(km, jm, im).transpose(2, 1, 0), ndwet.reshape(km, jm, im).transpose(2, 1, 0)


# ---- selected gridcells (include/ohxgb.h part 2: OHXSelectCells, OHXGatherCells, OHXScatterCells) ----
# bits of the device forms' status word
CELLS_OUT_OF_RANGE, CELLS_NOT_ASCENDING, CELLS_OVER_CAP = 1, 2, 4


def _flat_field(a) -> np.ndarray:
    """A field as the C ABI reads it: float32, Fortran order.  1-D arrays are taken as already flattened that way,
    [i,j(,k)]-indexed ones are flattened."""
    a = np.asarray(a, dtype=np.float32)
    return np.ascontiguousarray(a) if a.ndim == 1 else np.ascontiguousarray(a.ravel(order="F"))


def select_cells(im: int, jm: int, km: int, box=None, a=None, b=None, b0: float = 0.0, cap: Optional[int] = None,
                 out: Optional[np.ndarray] = None, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """OHXSelectCells on host arrays: the cell indices c = (i-1) + im*((j-1) + jm*(k-1)) of the box (i1, i2, j1, j2, k1,
    k2; 1-based, inclusive; default the whole block) with a > b, ascending, as an int64 array.  `a`, `b`: fields of
    im*jm*km elements, or of im*jm (2-D, the same on every level); b None: the scalar b0; a None: every cell of the
    box.  cap: most cells wanted (default: the box).  When more are selected the call raises OhxError, whose `count`
    attribute is the full count; `out`, an int64 array of at least cap entries, then holds the first cap."""
    lib = lib or load_library()
    i1, i2, j1, j2, k1, k2 = box or (1, im, 1, jm, 1, km)
    if cap is None:
        cap = max(0, i2 - i1 + 1) * max(0, j2 - j1 + 1) * max(0, k2 - k1 + 1)
    if out is None:
        out = np.empty(max(cap, 1), dtype=np.int64)
    elif out.dtype != np.int64 or not out.flags["C_CONTIGUOUS"] or out.size < cap:
        raise ValueError("out: a contiguous int64 array of at least cap entries")
    fa = _flat_field(a) if a is not None else None
    fb = _flat_field(b) if b is not None else None
    count = C.c_int64(0)
    rc = lib.OHXSelectCells(im, jm, km, i1, i2, j1, j2, k1, k2, fa.ctypes.data if fa is not None else None,
                            int(fa is not None and fa.size == im * jm), fb.ctypes.data if fb is not None else None,
                            int(fb is not None and fb.size == im * jm), b0, out.ctypes.data, cap, C.byref(count))
    if rc != 0:
        err = OhxError(lib.XGBGetLastError().decode("utf-8", "replace"))
        err.count = count.value
        raise err
    return out[:count.value].copy()


def select_cells_device(im: int, jm: int, km: int, box, a_ptr: int, a_is2d: bool, b_ptr: int, b_is2d: bool, b0: float,
                        cells_ptr: int, cap: int, count_ptr: int, status_ptr: int = 0, stream: int = 0,
                        lib: Optional[C.CDLL] = None) -> None:
    """OHXSelectCellsDevice: device addresses (a_ptr / b_ptr 0 for none; cells int64[cap], count int64[1], status
    uint32[1] or 0); only enqueues on `stream`."""
    lib = lib or load_library()
    i1, i2, j1, j2, k1, k2 = box or (1, im, 1, jm, 1, km)
    check(lib, lib.OHXSelectCellsDevice(im, jm, km, i1, i2, j1, j2, k1, k2, a_ptr or None, int(bool(a_is2d)),
                                        b_ptr or None, int(bool(b_is2d)), b0, cells_ptr or None, cap, count_ptr or None,
                                        status_ptr or None, stream or None))


def gather_cells(fields: Sequence[np.ndarray], is2d: Sequence[bool], pl_feature: int, im: int, jm: int, km: int, cells,
                 rows: Optional[np.ndarray] = None, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """OHXGatherCells on host arrays -> (ncell, nfield) float32: row n is what the fields forms gather for cell
    cells[n] (field pl_feature divided by 100; -1: none).  `rows`, when given, is filled even when the call raises
    (a cell out of range: its row is NaN)."""
    lib = lib or load_library()
    nf = len(fields)
    flat = [_flat_field(f) for f in fields]
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    if rows is None:
        rows = np.empty((cells.size, nf), dtype=np.float32)
    elif rows.dtype != np.float32 or not rows.flags["C_CONTIGUOUS"] or rows.size < cells.size * nf:
        raise ValueError("rows: a contiguous float32 array of ncell * nfield elements")
    ptrs = (C.c_void_p * max(nf, 1))(*[f.ctypes.data for f in flat])
    flags = (C.c_int32 * max(nf, 1))(*[1 if t else 0 for t in is2d])
    check(lib, lib.OHXGatherCells(ptrs, flags, nf, pl_feature, im, jm, km, cells.ctypes.data, cells.size,
                                  rows.ctypes.data))
    return rows


def gather_cells_device(field_ptrs: Sequence[int], is2d: Sequence[bool], pl_feature: int, im: int, jm: int, km: int,
                        cells_ptr: int, ncell: int, rows_ptr: int, status_ptr: int = 0, stream: int = 0,
                        lib: Optional[C.CDLL] = None) -> None:
    """OHXGatherCellsDevice: device addresses; rows float32[ncell][nfield]; only enqueues on `stream`."""
    lib = lib or load_library()
    nf = len(field_ptrs)
    ptrs = (C.c_void_p * max(nf, 1))(*field_ptrs)
    flags = (C.c_int32 * max(nf, 1))(*[1 if t else 0 for t in is2d])
    check(lib, lib.OHXGatherCellsDevice(ptrs, flags, nf, pl_feature, im, jm, km, cells_ptr or None, ncell,
                                        rows_ptr or None, status_ptr or None, stream or None))


def scatter_cells(values, col: int, cells, out3d: np.ndarray, im: int, jm: int, km: int,
                  lib: Optional[C.CDLL] = None) -> None:
    """OHXScatterCells on host arrays: out3d[cells[n]] = values[n, col] (values 1-D: col 0).  out3d: a writable float32
    array of im*jm*km elements in Fortran order (1-D, or F-contiguous 3-D); other cells keep what they hold."""
    lib = lib or load_library()
    values = np.ascontiguousarray(values, dtype=np.float32)
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    stride = 1 if values.ndim == 1 else values.shape[1]
    if (out3d.dtype != np.float32 or not out3d.flags["WRITEABLE"] or out3d.size < im * jm * km or
            not (out3d.flags["F_CONTIGUOUS"] or out3d.ndim == 1)):
        raise ValueError("out3d: a writable Fortran-order float32 array of im * jm * km elements")
    check(lib, lib.OHXScatterCells(values.ctypes.data, stride, col, cells.ctypes.data, cells.size, out3d.ctypes.data,
                                   im, jm, km))


def scatter_cells_device(values_ptr: int, stride: int, col: int, cells_ptr: int, ncell: int, out_ptr: int, im: int,
                         jm: int, km: int, status_ptr: int = 0, stream: int = 0, lib: Optional[C.CDLL] = None) -> None:
    """OHXScatterCellsDevice: device addresses; only enqueues on `stream`."""
    lib = lib or load_library()
    check(lib, lib.OHXScatterCellsDevice(values_ptr or None, stride, col, cells_ptr or None, ncell, out_ptr or None,
                                         im, jm, km, status_ptr or None, stream or None))


UNIQUE_ID_BYTES = 128


def quantile_cuts(x, missing: float = float("nan"), max_bins: int = 255, lib: Optional[C.CDLL] = None):
    """OHXQuantileCuts (host only) -> (cut_ptr uint64 [ncol + 1], cut_values float32): per column of the row-major
    sample `x` at most max_bins - 1 ascending cut values, what Booster.boost_trees takes as `cuts`."""
    lib = lib or load_library()
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.ndim == 2
    nrow, ncol = x.shape
    cut_ptr = np.zeros(ncol + 1, dtype=np.uint64)
    cap = ncol * (max_bins - 1) if 2 <= max_bins <= 255 else 0
    values = np.zeros(max(cap, 1), dtype=np.float32)
    needed = C.c_uint64()
    check(lib, lib.OHXQuantileCuts(x.ctypes.data, nrow, ncol, missing, max_bins, cut_ptr.ctypes.data, values.ctypes.data,
                                   cap, C.byref(needed)))
    return cut_ptr, values[:needed.value].copy()


def shard_rows(n_total: int, nranks: int, rank: int, lib: Optional[C.CDLL] = None):
    """OHXShardRows -> (row0, nrows)."""
    lib = lib or load_library()
    r0, n = C.c_uint64(), C.c_uint64()
    check(lib, lib.OHXShardRows(n_total, nranks, rank, C.byref(r0), C.byref(n)))
    return r0.value, n.value


class Communicator:
    """OHXCommInitRank handle: the RCCL communicator a Fortran/MPI host would build through the C ABI.
    `unique_id` = the 128 bytes rank 0 got from Communicator.unique_id(), distributed by the caller."""

    def __init__(self, unique_id: bytes, nranks: int, rank: int, lib: Optional[C.CDLL] = None):
        self.lib = lib or load_library()
        self.handle = C.c_void_p()
        self.nranks, self.rank = nranks, rank
        buf = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        check(self.lib, self.lib.OHXCommInitRank(C.cast(buf, C.c_void_p), nranks, rank, C.byref(self.handle)))

    @staticmethod
    def unique_id(lib: Optional[C.CDLL] = None) -> bytes:
        lib = lib or load_library()
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        check(lib, lib.OHXCommGetUniqueId(C.cast(buf, C.c_void_p)))
        return buf.raw

    @staticmethod
    def rccl_version(lib: Optional[C.CDLL] = None) -> int:
        """ncclGetVersion's code of the librccl.so the library loaded (e.g. 22705 for 2.27.5)."""
        lib = lib or load_library()
        v = C.c_int()
        check(lib, lib.OHXCommInfo(C.byref(v)))
        return v.value

    def all_gather_oh(self, shard_ptr: int, n_local: int, n_total: int, full_ptr: int, stream: int = 0) -> None:
        check(self.lib, self.lib.OHXAllGatherOH(self.handle, shard_ptr, n_local, n_total, full_ptr, stream or None))

    def free(self) -> None:
        if self.handle:
            check(self.lib, self.lib.OHXCommFree(self.handle))
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_count() -> int:
    lib = load_library()
    n = C.c_int()
    check(lib, lib.OHXDeviceCount(C.byref(n)))
    return n.value
