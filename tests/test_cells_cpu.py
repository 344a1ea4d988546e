"""Selected gridcells (OHXSelectCells, OHXGatherCells, OHXScatterCells), what can be checked without a GPU: the six
symbols are declared, bound and exported; every argument refusal and its message, in both forms; the host forms fail
loudly without a device; cells.hip cross-compiles for gfx950 with no scratch and no flat memory instructions; the LDS
stride of the gather puts a wave's transposing writes on different banks; the numpy restatement of
tests/cells_support.py agrees with plain loops on a 5 x 3 x 4 grid; the Fortran driver links the product only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import cells_support as cs
from tests import helpers

HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["select_count_kernel", "select_write_kernel", "gather_cells_kernel", "scatter_max_kernel",
           "scatter_write_kernel"]
SYMBOLS = ["OHXSelectCells", "OHXSelectCellsDevice", "OHXGatherCells", "OHXGatherCellsDevice", "OHXScatterCells",
           "OHXScatterCellsDevice"]
GRID = (5, 3, 4)


# ---- the ABI ----

def test_entry_points_declared_bound_and_exported():
    lib = C.CDLL(helpers.PRODUCT_SO)
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name), name
    bindings = open(os.path.join(helpers.ROOT, "quickchem_amd", "fortran", "ohx_bindings.F90")).read()
    for name in SYMBOLS:
        assert f'bind(C, name="{name}")' in bindings, name
    for name in ("select_cells", "gather_cells", "scatter_cells"):
        assert hasattr(capi, name) and hasattr(capi, name + "_device")
    assert hasattr(capi.Booster, "explain_cells")
    assert (capi.CELLS_OUT_OF_RANGE, capi.CELLS_NOT_ASCENDING, capi.CELLS_OVER_CAP) == (1, 2, 4)
    for name, bit in (("OHX_CELLS_OUT_OF_RANGE", 1), ("OHX_CELLS_NOT_ASCENDING", 2), ("OHX_CELLS_OVER_CAP", 4)):
        assert re.search(r"#define " + name + r" " + str(bit) + r"u\b", header)


def test_fortran_driver_is_built_against_the_product_only():
    exe = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "cells_driver_hip")
    assert os.path.exists(exe), exe
    out = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True).stdout
    assert "libohxgb.so" in out and "oracle" not in out
    nm = subprocess.run(["nm", "-D", "--undefined-only", exe], stdout=subprocess.PIPE, text=True).stdout
    assert "OHXSelectCells" in nm and "OHXGatherCells" in nm
    # the oracle-linked drivers link ohx_bindings.o too: the interface blocks alone must not pull the symbols in
    obj = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "obj", "ohx_bindings.o")
    nm = subprocess.run(["nm", "--undefined-only", obj], stdout=subprocess.PIPE, text=True).stdout
    assert "Cells" not in nm


# ---- refusals: raised before a device is looked for, so the same with and without one ----

def fields_of(n, grid=GRID, two_d=()):
    im, jm, km = grid
    return [np.zeros(im * jm if f in two_d else im * jm * km, dtype=np.float32) for f in range(n)]


ONE = np.zeros(1, dtype=np.int64)


def select_host(grid, box, cap=4, cells=ONE, count=True, a=None):
    lib = capi.load_library()
    n = C.c_int64()
    return lib.OHXSelectCells(*grid, *box, a, 0, None, 0, 0.0, cells.ctypes.data if cells is not None else None, cap,
                              C.byref(n) if count else None)


def select_device(grid, box, cap=4, cells=8, count=8):
    lib = capi.load_library()
    return lib.OHXSelectCellsDevice(*grid, *box, None, 0, None, 0, 0.0, cells, cap, count, None, None)


@pytest.mark.parametrize("call", [select_host, select_device])
def test_selection_refusals(call):
    lib = capi.load_library()
    ok_box = (1, 5, 1, 3, 1, 4)
    for grid in ((0, 3, 4), (5, -1, 4), (5, 3, 0)):
        assert call(grid, ok_box) == -1
        assert lib.XGBGetLastError() == b"predict_fields: im, jm, km must be positive"
    for box in ((0, 5, 1, 3, 1, 4), (1, 6, 1, 3, 1, 4), (3, 1, 1, 3, 1, 4), (1, 5, 0, 3, 1, 4), (1, 5, 1, 4, 1, 4),
                (1, 5, 3, 1, 1, 4), (1, 5, 1, 3, 0, 4), (1, 5, 1, 3, 1, 5), (1, 5, 1, 3, 4, 2)):
        assert call(GRID, box) == -1, box
        assert lib.XGBGetLastError() == b"select_cells: need 1 <= i1, i2 <= im, i2 >= i1 - 1, and the same for j and k"
    assert call(GRID, ok_box, cap=-1) == -1
    assert lib.XGBGetLastError() == b"select_cells: cap must not be negative"
    assert call(GRID, ok_box, cells=None) == -1
    assert lib.XGBGetLastError() == b"select_cells: NULL argument"
    assert call(GRID, ok_box, count=None) == -1
    assert lib.XGBGetLastError() == b"select_cells: NULL argument"


def test_an_empty_box_needs_no_device():
    """i2 == i1 - 1 and the like: nothing selected, success - the host form does not even look for a device."""
    for box in ((3, 2, 1, 3, 1, 4), (1, 5, 2, 1, 1, 4), (1, 5, 1, 3, 5, 4), (1, 0, 1, 0, 1, 0)):
        assert capi.select_cells(*GRID, box=box).size == 0
    assert capi.gather_cells(fields_of(2), [0, 0], -1, *GRID, []).shape == (0, 2)
    out = np.full(60, 7.0, dtype=np.float32)
    capi.scatter_cells(np.zeros((0, 3), dtype=np.float32), 1, [], out, *GRID)
    assert np.all(out == 7.0)


def gather_call(device, fields, is2d, nfield, grid, cells, ncell, rows, pl=-1):
    lib = capi.load_library()
    ptrs = (C.c_void_p * 33)(*[f.ctypes.data if f is not None else None for f in fields]) if fields is not None else None
    flags = (C.c_int32 * 33)(*is2d) if is2d is not None else None
    c = cells.ctypes.data if cells is not None else None
    r = rows.ctypes.data if rows is not None else None
    if device:
        return lib.OHXGatherCellsDevice(ptrs, flags, nfield, pl, *grid, c, ncell, r, None, None)
    return lib.OHXGatherCells(ptrs, flags, nfield, pl, *grid, c, ncell, r)


@pytest.mark.parametrize("device", [False, True])
def test_gather_refusals(device):
    lib = capi.load_library()
    cells, rows = np.zeros(2, dtype=np.int64), np.zeros(2 * 33, dtype=np.float32)
    f33 = fields_of(33)
    for nfield in (0, -1, 33):
        assert gather_call(device, f33, [0] * 33, nfield, GRID, cells, 2, rows) == -1
        assert lib.XGBGetLastError() == b"gather_cells: nfield must be 1..32"
    for grid in ((0, 3, 4), (5, 0, 4), (5, 3, -2)):
        assert gather_call(device, f33, [0] * 33, 27, grid, cells, 2, rows) == -1
        assert lib.XGBGetLastError() == b"predict_fields: im, jm, km must be positive"
    assert gather_call(device, f33, [0] * 33, 27, GRID, cells, -1, rows) == -1
    assert lib.XGBGetLastError() == b"gather_cells: ncell must not be negative"
    for kw in (dict(fields=None), dict(is2d=None), dict(cells=None), dict(rows=None)):
        args = dict(fields=f33, is2d=[0] * 33, cells=cells, rows=rows)
        args.update(kw)
        assert gather_call(device, args["fields"], args["is2d"], 27, GRID, args["cells"], 2, args["rows"]) == -1, kw
        assert lib.XGBGetLastError() == b"predict_fields: NULL argument"
    holed = list(f33)
    holed[5] = None
    assert gather_call(device, holed, [0] * 33, 27, GRID, cells, 2, rows) == -1
    assert lib.XGBGetLastError() == b"predict_fields: field 5 is NULL"


@pytest.mark.parametrize("device", [False, True])
def test_scatter_refusals(device):
    lib = capi.load_library()
    values, cells, out = np.zeros(6, dtype=np.float32), np.zeros(2, dtype=np.int64), np.zeros(60, dtype=np.float32)

    def call(v=values, stride=3, col=0, c=cells, ncell=2, o=out, grid=GRID):
        p = [a.ctypes.data if a is not None else None for a in (v, c, o)]
        if device:
            return lib.OHXScatterCellsDevice(p[0], stride, col, p[1], ncell, p[2], *grid, None, None)
        return lib.OHXScatterCells(p[0], stride, col, p[1], ncell, p[2], *grid)

    assert call(grid=(5, 3, 0)) == -1
    assert lib.XGBGetLastError() == b"predict_fields: im, jm, km must be positive"
    assert call(ncell=-1) == -1
    assert lib.XGBGetLastError() == b"scatter_cells: ncell must not be negative"
    for stride, col in ((0, 0), (3, 3), (3, -1), (-2, 0)):
        assert call(stride=stride, col=col) == -1
        assert lib.XGBGetLastError() == b"scatter_cells: need stride >= 1 and 0 <= col < stride"
    for kw in (dict(v=None), dict(c=None), dict(o=None)):
        assert call(**kw) == -1, kw
        assert lib.XGBGetLastError() == b"scatter_cells: NULL argument"


def test_host_forms_fail_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(capi.OhxError, match="no CPU fallback"):
        capi.select_cells(*GRID)
    with pytest.raises(capi.OhxError, match="no CPU fallback"):
        capi.gather_cells(fields_of(3), [0, 0, 0], 1, *GRID, [0, 7])
    with pytest.raises(capi.OhxError, match="no CPU fallback"):
        capi.scatter_cells(np.zeros((2, 1), dtype=np.float32), 0, [0, 7], np.zeros(60, dtype=np.float32), *GRID)
    # and the device forms
    with pytest.raises(capi.OhxError, match="no CPU fallback"):
        capi.select_cells_device(*GRID, None, 0, False, 0, False, 0.0, 8, 4, 8)
    with pytest.raises(capi.OhxError, match="no CPU fallback"):
        capi.gather_cells_device([8, 8], [0, 0], -1, *GRID, 8, 2, 8)
    with pytest.raises(capi.OhxError, match="no CPU fallback"):
        capi.scatter_cells_device(8, 1, 0, 8, 2, 8, *GRID)


# ---- the kernels' ISA ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "cells.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "cells.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel_body(text, name_part):
    m = re.search(r"^(_Z\w*" + re.escape(name_part) + r"\w*):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, name_part
    return m.group(2)


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernels_have_no_scratch_and_no_flat_access(isa, kernel):
    body = kernel_body(isa, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0


def test_gather_stores_through_lds(isa):
    """The rows leave through LDS: one float per lane and store, 64 consecutive floats per instruction - no lane
    stores a row of its own."""
    body = kernel_body(isa, "gather_cells_kernel")
    assert "ds_write_b32" in body and "ds_read_b32" in body
    assert len(re.findall(r"global_store_dword\b", body)) == 1
    assert not re.search(r"global_store_dwordx[234]", body)


# ---- launch shapes ----

@pytest.mark.parametrize("nfield", range(1, 33))
def test_gather_lds_stride_keeps_transposing_writes_off_each_others_banks(nfield):
    """ds_write_b32 serves a wave in two groups of 32 lanes over banks = dword address mod 32 (the same holds for 64
    banks and all 64 lanes): lane l writes its row's column f at l * stride + f."""
    stride = synth.cells_plan(64, nfield)[2]
    assert stride >= nfield and stride <= nfield + 1
    for f in (0, nfield - 1):
        for lanes, banks in ((range(0, 32), 32), (range(32, 64), 32), (range(64), 64)):
            assert len({(l * stride + f) % banks for l in lanes}) == len(lanes)


def test_pass_plan():
    assert synth.cells_plan(0)[:2] == (0, 0)
    assert synth.cells_plan(60)[:2] == (1, 256)
    blocks, chunk = synth.cells_plan(96 * 48 * 6)[:2]
    assert blocks > 1 and chunk % 256 == 0 and blocks * chunk >= 96 * 48 * 6 > (blocks - 1) * chunk
    blocks, chunk = synth.cells_plan(360 * 2160 * 72)[:2]
    assert blocks <= 4096 and chunk % 256 == 0 and blocks * chunk >= 360 * 2160 * 72 > (blocks - 1) * chunk
    assert synth.cells_plan(4097)[3] == 65


# ---- the restatement against plain loops ----

@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(5)
    im, jm, km = GRID
    a3 = rng.normal(size=GRID).astype(np.float32)
    b3 = rng.normal(size=GRID).astype(np.float32)
    a2 = rng.normal(size=GRID[:2]).astype(np.float32)
    b2 = rng.normal(size=GRID[:2]).astype(np.float32)
    a3[1, 1, 1] = np.nan
    b3[2, 2, 2] = np.nan
    b3[0, 0, 0] = a3[0, 0, 0]
    return a3, b3, a2, b2


def test_selection_restatement_against_loops(small):
    a3, b3, a2, b2 = small
    boxes = [cs.whole(*GRID), (2, 4, 1, 2, 2, 3), (3, 3, 2, 2, 1, 4), (1, 5, 1, 3, 3, 2), (5, 5, 3, 3, 4, 4)]
    for box in boxes:
        for a in (None, a3, a2):
            for b in (None, b3, b2):
                got = cs.select(*GRID, box, a, b, 0.25)
                want = cs.select_loops(*GRID, box, a, b, 0.25)
                assert np.array_equal(got, want), (box, a is None, b is None)
                assert np.all(np.diff(got) > 0)
    assert np.array_equal(cs.select(*GRID, cs.whole(*GRID)), np.arange(60))
    assert 0 not in cs.select(*GRID, cs.whole(*GRID), a3, b3)           # equal on both sides: not selected


def test_gather_restatement_against_loops():
    rng = np.random.default_rng(6)
    is2d = [True, False, False, True, False]
    fields = [rng.normal(size=GRID[:2] if t else GRID).astype(np.float32) * 1000 for t in is2d]
    fields[1][0, 0, 0], fields[2][1, 1, 1], fields[2][2, 2, 2] = -999.0, np.nan, np.inf
    cells = np.array([59, 0, 7, 7, -1, 60, 31, 2 ** 40, 16], dtype=np.int64)
    for pl in (-1, 1, 3):
        got, gs = cs.gather(fields, is2d, pl, *GRID, cells)
        want, ws = cs.gather_loops(fields, is2d, pl, *GRID, cells)
        assert np.array_equal(helpers.bits(got), helpers.bits(want)) and gs == ws == cs.OUT_OF_RANGE
    got, gs = cs.gather(fields, is2d, 1, *GRID, cells[:4])
    assert gs == 0 and got[1, 1] == np.float32(-999.0) / np.float32(100)


def test_scatter_restatement_against_loops():
    rng = np.random.default_rng(7)
    out0 = np.full(60, -5.0, dtype=np.float32)
    lists = [[0, 3, 59], [], [5, 3, 5, 9], [0, 5, 3, 4, 9], [4, 4], [-3, 2, 60, 7], [10, 2 ** 40, 11, 12], [59, 0]]
    for cells in lists:
        values = rng.normal(size=(len(cells), 3)).astype(np.float32)
        got, gs = cs.scatter(values, 1, cells, out0, 60)
        want, ws = cs.scatter_loops(values, 1, cells, out0, 60)
        assert np.array_equal(helpers.bits(got), helpers.bits(want)) and gs == ws, cells
    # no cell is written twice: [5, 3, 5, 9] keeps the FIRST 5's value
    values = np.arange(12, dtype=np.float32).reshape(4, 3)
    got, status = cs.scatter(values, 0, [5, 3, 5, 9], out0, 60)
    assert got[5] == 0.0 and got[3] == -5.0 and got[9] == 9.0 and status == cs.NOT_ASCENDING
