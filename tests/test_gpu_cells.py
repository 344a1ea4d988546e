"""Selected gridcells on the GPU (OHXSelectCells, OHXGatherCells, OHXScatterCells; csrc/cells.hip), host and device
forms, against the numpy restatement of tests/cells_support.py - bit for bit: uint32 views of floats, array_equal of
indices.  Then what the calls are for: the rows forms on a gathered matrix give the fields forms' bits at the selected
cells; interactions, a categorical and a three-group booster run on gathered rows; the Fortran driver; explain_cells."""
import os

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import categorical_support as catsup
from tests import cells_support as cs
from tests import helpers
from tests import output_groups_support as og

pytestmark = pytest.mark.gpu

SMALL, LARGE = (5, 3, 4), (96, 48, 6)
SENTINEL = np.uint32(0x7FC0DEAD)          # a quiet NaN with a payload: nothing the kernels compute
UNTOUCHED = -7                            # what the cells buffer holds where nothing was written
DRIVER = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "cells_driver_hip")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def fflat(a):
    """[i,j(,k)]-indexed -> the Fortran-order buffer the C ABI reads."""
    return np.ascontiguousarray(np.asarray(a).ravel(order="F"))


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinels(torch, n):
    return to_dev(torch, np.full(n, SENTINEL, dtype=np.uint32).view(np.int32)).view(torch.float32)


def select_device(torch, grid, box, a, b, b0, cap=None):
    """-> (the whole cells buffer of cap entries, count, status)"""
    im, jm, km = grid
    if cap is None:
        cap = im * jm * km
    da = to_dev(torch, fflat(a)) if a is not None else None
    db = to_dev(torch, fflat(b)) if b is not None else None
    cells = torch.full((max(cap, 1),), UNTOUCHED, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.select_cells_device(im, jm, km, box, da.data_ptr() if a is not None else 0, a is not None and a.ndim == 2,
                             db.data_ptr() if b is not None else 0, b is not None and b.ndim == 2, b0,
                             cells.data_ptr(), cap, count.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    return cells.cpu().numpy()[:cap], int(count.item()), int(status.item())


# ---- 1. selection ----

def selection_cases(grid):
    """(name, box, a, b, b0): a and b each 3-D, 2-D and absent; nothing, everything, the first and the last cell alone,
    a column, masks at two densities, NaN on either side, equal values, a box that cuts the grid three ways."""
    im, jm, km = grid
    rng = np.random.default_rng(im * 1000 + km)
    whole = cs.whole(*grid)
    cut = (2, 4, 2, 3, 2, 3) if grid == SMALL else (3, 72, 5, 40, 2, 5)          # LARGE: 70 wide, no multiple of 64
    zeros, ones = np.zeros(grid, dtype=np.float32), np.ones(grid, dtype=np.float32)
    first, last = zeros.copy(), zeros.copy()
    first[0, 0, 0], last[-1, -1, -1] = 1.0, 1.0
    cases = [("nothing", whole, zeros, None, 0.0), ("everything", whole, ones, None, 0.0),
             ("everything, no field", whole, None, None, 0.0), ("first", whole, first, None, 0.0),
             ("last", whole, last, None, 0.0), ("column", (im, im, 2, 2, 1, km), None, None, 0.0),
             ("cut box, no field", cut, None, None, 0.0)]
    for density in (0.3, 0.01):
        mask = (rng.random(grid) < density).astype(np.float32)
        cases.append((f"mask {density}", whole, mask, None, 0.0))
        cases.append((f"mask {density} in the cut box", cut, mask, None, 0.0))
    for a_dim in (3, 2):
        for b_dim in (3, 2, None):
            a = rng.normal(size=grid[:a_dim]).astype(np.float32)
            b = rng.normal(size=grid[:b_dim]).astype(np.float32) if b_dim else None
            a[rng.random(a.shape) < 0.05] = np.nan
            if b is not None:
                b[rng.random(b.shape) < 0.05] = np.nan
                same = rng.random(grid) < 0.1                      # equal on both sides: not selected
                a3 = np.broadcast_to(a[:, :, None] if a_dim == 2 else a, grid)
                if b_dim == 3:
                    b[same] = a3[same]
                elif a_dim == 2:
                    b[same[:, :, 0]] = a[same[:, :, 0]]
            b0 = float(a.flat[3]) if not np.isnan(a.flat[3]) else 0.25      # a value a holds: equal there
            for box in (whole, cut):
                cases.append((f"a {a_dim}-D, b {b_dim}-D, box {box}", box, a, b, b0))
    return cases


@pytest.mark.parametrize("grid", [SMALL, LARGE])
def test_selection_device_and_host(torch_cuda, grid):
    total = grid[0] * grid[1] * grid[2]
    if grid == LARGE:
        assert synth.cells_plan(total)[0] > 1                      # more than one block: the offsets come from the scan
    seen = set()
    for name, box, a, b, b0 in selection_cases(grid):
        want = cs.select(*grid, box, a, b, b0)
        seen.add(min(want.size, 2) if want.size < total else "all")
        buf, count, status = select_device(torch_cuda, grid, box, a, b, b0)
        assert count == want.size and status == 0, name
        assert np.array_equal(buf[:count], want), name
        assert np.all(buf[count:] == UNTOUCHED), name
        got = capi.select_cells(*grid, box=box, a=a, b=b, b0=b0)
        assert np.array_equal(got, want), name
    assert seen == {0, 1, 2, "all"}


@pytest.mark.parametrize("grid", [SMALL, LARGE])
def test_selection_cap_and_empty_box(torch_cuda, grid):
    im, jm, km = grid
    rng = np.random.default_rng(9)
    a = rng.normal(size=grid).astype(np.float32)
    b = rng.normal(size=grid[:2]).astype(np.float32)
    box = cs.whole(*grid)
    want = cs.select(*grid, box, a, b)
    assert want.size > 2
    # cap exactly the count
    buf, count, status = select_device(torch_cuda, grid, box, a, b, 0.0, cap=want.size)
    assert count == want.size and status == 0 and np.array_equal(buf, want)
    assert np.array_equal(capi.select_cells(*grid, a=a, b=b, cap=want.size), want)
    # one less: the prefix, the full count, the bit
    buf, count, status = select_device(torch_cuda, grid, box, a, b, 0.0, cap=want.size - 1)
    assert count == want.size and status == cs.OVER_CAP and np.array_equal(buf, want[:-1])
    out = np.full(want.size - 1, UNTOUCHED, dtype=np.int64)
    with pytest.raises(capi.OhxError, match=f"{want.size} cells are selected and cap is {want.size - 1}") as e:
        capi.select_cells(*grid, a=a, b=b, cap=want.size - 1, out=out)
    assert e.value.count == want.size and np.array_equal(out, want[:-1])
    # cap 0
    buf, count, status = select_device(torch_cuda, grid, box, a, b, 0.0, cap=0)
    assert count == want.size and status == cs.OVER_CAP
    # empty boxes: nothing, success, the count written
    for empty in ((3, 2, 1, jm, 1, km), (1, im, 2, 1, 1, km), (1, im, 1, jm, km + 1, km)):
        buf, count, status = select_device(torch_cuda, grid, empty, a, b, 0.0)
        assert count == 0 and status == 0 and np.all(buf == UNTOUCHED)
        assert capi.select_cells(*grid, box=empty, a=a, b=b).size == 0


def test_selection_twice_gives_the_same_array(torch_cuda):
    rng = np.random.default_rng(10)
    a = (rng.random(LARGE) < 0.3).astype(np.float32)
    one = select_device(torch_cuda, LARGE, cs.whole(*LARGE), a, None, 0.0)
    two = select_device(torch_cuda, LARGE, cs.whole(*LARGE), a, None, 0.0)
    assert one[1] == two[1] > 0 and np.array_equal(one[0], two[0])


# ---- 2. gather ----

GATHER_GRID = (12, 6, 8)


def gather_fields(nfield, seed):
    """nfield fields on GATHER_GRID, every third one 2-D, salted with -999, NaN and +-inf; values whose division by 100
    is inexact."""
    rng = np.random.default_rng(seed)
    is2d = [f % 3 == 0 for f in range(nfield)]
    fields = []
    for f in range(nfield):
        a = (rng.normal(size=GATHER_GRID[:2] if is2d[f] else GATHER_GRID) * 1013.25 + 50000.0 / 7.0).astype(np.float32)
        salt = rng.random(a.shape)
        a[salt < 0.03] = -999.0
        a[(salt >= 0.03) & (salt < 0.06)] = np.nan
        a[(salt >= 0.06) & (salt < 0.08)] = np.inf
        a[(salt >= 0.08) & (salt < 0.10)] = -np.inf
        fields.append(a)
    return fields, is2d


def gather_device(torch, fields, is2d, pl, grid, cells):
    dev_fields = [to_dev(torch, fflat(f)) for f in fields]
    n, nf = len(cells), len(fields)
    d_cells = to_dev(torch, np.asarray(cells, dtype=np.int64)) if n else torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = sentinels(torch, max(n, 1) * nf + 64)                 # 64 more: nothing is written past the last row
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.gather_cells_device([t.data_ptr() for t in dev_fields], is2d, pl, *grid, d_cells.data_ptr(), n,
                             rows.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    got = helpers.bits(rows.cpu().numpy())
    assert np.all(got[n * nf:] == SENTINEL)
    return got[:n * nf].reshape(n, nf), int(status.item())


def cell_lists(ncell, total, seed):
    rng = np.random.default_rng(seed)
    if ncell <= total:
        asc = np.sort(rng.choice(total, size=ncell, replace=False)).astype(np.int64)
    else:
        asc = np.sort(rng.integers(0, total, size=ncell)).astype(np.int64)
    return {"ascending": asc, "shuffled": rng.permutation(asc), "duplicates": rng.integers(0, total, size=ncell)}


@pytest.mark.parametrize("nfield", [1, 27, 32])
@pytest.mark.parametrize("ncell", [0, 1, 63, 64, 65, 4097])
def test_gather_against_the_restatement(torch_cuda, nfield, ncell):
    grid = GATHER_GRID
    total = grid[0] * grid[1] * grid[2]
    fields, is2d = gather_fields(nfield, 100 + nfield)
    for order, cells in cell_lists(ncell, total, ncell).items():
        for pl in ((1 if nfield > 1 else 0), -1):
            want, _ = cs.gather(fields, is2d, pl, *grid, cells)
            got, status = gather_device(torch_cuda, fields, is2d, pl, grid, cells)
            assert status == 0 and np.array_equal(got, helpers.bits(want)), (order, pl)
        if order == "shuffled":
            host = capi.gather_cells(fields, is2d, pl, *grid, cells)
            assert np.array_equal(helpers.bits(host), helpers.bits(want))
    if ncell >= 63 and nfield > 1:
        rows, _ = cs.gather(fields, is2d, 1, *grid, cell_lists(ncell, total, ncell)["ascending"])
        for special in (-999.0, np.inf, -np.inf):                       # they pass through unchanged
            assert (rows[:, [f for f in range(nfield) if f != 1]] == np.float32(special)).any()
        assert np.isnan(rows).any()
        pl_in = fflat(fields[1])[cell_lists(ncell, total, ncell)["ascending"]]
        ok = np.isfinite(pl_in) & (pl_in != -999.0)
        assert (rows[ok, 1].astype(np.float64) * 100.0 != pl_in[ok].astype(np.float64)).any()       # inexact divisions


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("bad", [-1, 12 * 6 * 8, -2 ** 40, 2 ** 40])
def test_gather_a_cell_out_of_range_is_a_nan_row(torch_cuda, where, bad):
    grid = GATHER_GRID
    fields, is2d = gather_fields(5, 77)
    cells = cell_lists(130, 576, 3)["shuffled"].copy()
    at = {"first": 0, "middle": 64, "last": 129}[where]
    cells[at] = bad
    want, wstatus = cs.gather(fields, is2d, 1, *grid, cells)
    assert wstatus == cs.OUT_OF_RANGE and np.isnan(want[at]).all()
    got, status = gather_device(torch_cuda, fields, is2d, 1, grid, cells)
    assert status == cs.OUT_OF_RANGE and np.array_equal(got, helpers.bits(want))
    rows = np.zeros((130, 5), dtype=np.float32)
    with pytest.raises(capi.OhxError, match=f"out of range at position {at} "):
        capi.gather_cells(fields, is2d, 1, *grid, cells, rows=rows)
    assert np.array_equal(helpers.bits(rows), helpers.bits(want))


# ---- 3. scatter ----

def scatter_device(torch, values, col, cells, out0, grid):
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(len(cells), -1)
    d_values = to_dev(torch, values) if values.size else torch.zeros(1, device="cuda")
    d_cells = (to_dev(torch, np.asarray(cells, dtype=np.int64)) if len(cells) else
               torch.zeros(1, dtype=torch.int64, device="cuda"))
    d_out = to_dev(torch, out0.copy())
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.scatter_cells_device(d_values.data_ptr(), values.shape[1], col, d_cells.data_ptr(), len(cells),
                              d_out.data_ptr(), *grid, status.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("grid,ncell", [(SMALL, 17), (LARGE, 4097)])
def test_scatter_round_trip(torch_cuda, grid, ncell):
    """Gather one field alone, scatter it into an array of sentinels: the field at the cells, the sentinel elsewhere."""
    total = grid[0] * grid[1] * grid[2]
    rng = np.random.default_rng(ncell)
    field = rng.normal(size=grid).astype(np.float32)
    cells = cell_lists(ncell, total, 4)["ascending"]
    assert ncell <= 256 or synth.cells_plan(ncell)[0] > 1                # the large list takes several blocks
    rows, status = gather_device(torch_cuda, [field], [False], -1, grid, cells)
    assert status == 0
    out0 = np.full(total, SENTINEL, dtype=np.uint32).view(np.float32)
    got, status = scatter_device(torch_cuda, rows.view(np.float32), 0, cells, out0, grid)
    want = out0.copy()
    want[cells] = fflat(field)[cells]
    assert status == 0 and np.array_equal(helpers.bits(got), helpers.bits(want))
    host = out0.copy()
    capi.scatter_cells(rows.view(np.float32), 0, cells, host, *grid)
    assert np.array_equal(helpers.bits(host), helpers.bits(want))
    # a column of a wider matrix
    wide = rng.normal(size=(ncell, 3)).astype(np.float32)
    wide[:, 2] = rows.view(np.float32)[:, 0]
    got, status = scatter_device(torch_cuda, wide, 2, cells, out0, grid)
    assert status == 0 and np.array_equal(helpers.bits(got), helpers.bits(want))


def bad_lists(total):
    asc = cell_lists(700, total, 8)["ascending"]
    swapped = asc.copy()
    swapped[[255, 256]] = swapped[[256, 255]]                       # a descent across two blocks of the pass
    back = asc.copy()
    back[300] = asc[10]                                             # a cell again, far behind: not written twice
    low = asc.copy()
    low[400:420] = asc[100:120]                                     # a run that starts again from below
    return {"swapped": swapped, "repeated": back, "run from below": low, "equal neighbours": np.repeat(asc[:300], 2),
            "descending": asc[::-1].copy(), "short": np.array([5, 3, 5, 9], dtype=np.int64)}


@pytest.mark.parametrize("name", ["swapped", "repeated", "run from below", "equal neighbours", "descending", "short"])
def test_scatter_not_ascending(torch_cuda, name):
    grid = LARGE
    total = grid[0] * grid[1] * grid[2]
    cells = bad_lists(total)[name]
    values = np.random.default_rng(11).normal(size=(len(cells), 2)).astype(np.float32)
    out0 = np.full(total, SENTINEL, dtype=np.uint32).view(np.float32)
    want, wstatus = cs.scatter(values, 1, cells, out0, total)
    assert wstatus == cs.NOT_ASCENDING
    got, status = scatter_device(torch_cuda, values, 1, cells, out0, grid)
    assert status == cs.NOT_ASCENDING and np.array_equal(helpers.bits(got), helpers.bits(want))
    host = out0.copy()
    with pytest.raises(capi.OhxError, match="strictly ascending: position"):
        capi.scatter_cells(values, 1, cells, host, *grid)
    assert np.array_equal(helpers.bits(host), helpers.bits(want))


def test_scatter_out_of_range_is_skipped(torch_cuda):
    grid = SMALL
    cells = np.array([-2 ** 40, -1, 0, 7, 59, 60, 2 ** 40], dtype=np.int64)
    values = np.arange(7, dtype=np.float32) + 1
    out0 = np.full(60, SENTINEL, dtype=np.uint32).view(np.float32)
    want, wstatus = cs.scatter(values, 0, cells, out0, 60)
    assert wstatus == cs.OUT_OF_RANGE and want[0] == 3.0 and want[59] == 5.0
    got, status = scatter_device(torch_cuda, values, 0, cells, out0, grid)
    assert status == cs.OUT_OF_RANGE and np.array_equal(helpers.bits(got), helpers.bits(want))
    host = out0.copy()
    with pytest.raises(capi.OhxError, match="out of range at position 0 "):
        capi.scatter_cells(values, 0, cells, host, *grid)
    assert np.array_equal(helpers.bits(host), helpers.bits(want))


# ---- 4. the fields forms' bits ----

BLOCK = (12, 6, 8)
K1, K2 = 3, 6
NFIELD = 25                      # fewer fields than the booster has features: the rest are missing


@pytest.fixture(scope="module")
def contribs_model():
    """The synthetic OH recipe at 20 trees (depth <= 18, grown on C12)."""
    return synth.make_model(num_trees=20, max_depth=18, sample_log2=16, min_leaf=2, grid=synth.GRIDS["C12"])


@pytest.fixture(scope="module")
def block_state():
    """The synthetic state on BLOCK, -999 salted into the fields -> (pl, tropp, fields[NFIELD])."""
    pl, tropp, fields = helpers.synth_state(BLOCK)
    rng = np.random.default_rng(21)
    out = []
    for f in fields[:NFIELD]:
        f = np.array(f, dtype=np.float32)
        f[rng.random(f.shape) < 0.02] = np.float32(synth.XX_MISS)
        out.append(f)
    return np.array(pl), np.array(tropp), out


@pytest.fixture(scope="module")
def block_selection(torch_cuda, block_state):
    """The tropospheric cells of the slab (PL_MOD > TROPP, as OH Run1 masks), selected and gathered on the device ->
    (cells tensor, rows tensor, device fields)."""
    torch = torch_cuda
    pl, tropp, fields = block_state
    im, jm, km = BLOCK
    box = (1, im, 1, jm, K1, K2)
    buf, count, status = select_device(torch, BLOCK, box, pl, tropp, 0.0)
    want = cs.select(*BLOCK, box, pl, tropp)
    assert status == 0 and np.array_equal(buf[:count], want)
    assert 0 < count < im * jm * (K2 - K1 + 1)
    dev_fields = [to_dev(torch, fflat(f)) for f in fields]
    cells = to_dev(torch, want)
    rows = torch.empty((count, NFIELD), dtype=torch.float32, device="cuda")
    capi.gather_cells_device([t.data_ptr() for t in dev_fields], synth.IS2D[:NFIELD], synth.PL_FEATURE, *BLOCK,
                             cells.data_ptr(), count, rows.data_ptr())
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == np.float32(synth.XX_MISS)).any()
    return cells, rows, dev_fields


def test_margins_on_gathered_rows_are_the_fields_predict_s(torch_cuda, contribs_model, block_selection):
    torch = torch_cuda
    cells, rows, dev_fields = block_selection
    im, jm, km = BLOCK
    b = capi.Booster(model_buffer=contribs_model.image)
    total, slab0 = im * jm * km, im * jm * (K1 - 1)
    oh = torch.zeros(total, dtype=torch.float32, device="cuda")
    margin = torch.zeros(im * jm * (K2 - K1 + 1), dtype=torch.float32, device="cuda")
    b.predict_fields_device([t.data_ptr() for t in dev_fields], synth.IS2D[:NFIELD], synth.PL_FEATURE, *BLOCK, K1, K2,
                            synth.XX_MISS, oh.data_ptr(), margin_ptr=margin.data_ptr())
    dmat = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=rows.shape[0], ncol=NFIELD, missing=synth.XX_MISS)
    out = torch.zeros(rows.shape[0], dtype=torch.float32, device="cuda")
    b.predict_device(dmat, out.data_ptr(), option_mask=1)
    torch.cuda.synchronize()
    b.check()
    at = cells.cpu().numpy() - slab0
    assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(margin.cpu().numpy()[at]))


@pytest.mark.parametrize("approximate", [True, False])
def test_contribs_on_gathered_rows_are_the_fields_form_s(torch_cuda, contribs_model, block_selection, approximate):
    torch = torch_cuda
    cells, rows, dev_fields = block_selection
    im, jm, km = BLOCK
    total, ncell = im * jm * km, rows.shape[0]
    b = capi.Booster(model_buffer=contribs_model.image)
    from_fields = [sentinels(torch, total) for _ in range(28)]
    b.predict_contribs_fields_device([t.data_ptr() for t in dev_fields], synth.IS2D[:NFIELD], synth.PL_FEATURE, *BLOCK,
                                     K1, K2, synth.XX_MISS, [t.data_ptr() for t in from_fields],
                                     approximate=approximate)
    dmat = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=ncell, ncol=NFIELD, missing=synth.XX_MISS)
    phi = torch.zeros((ncell, 28), dtype=torch.float32, device="cuda")
    b.predict_contribs_device(dmat, phi.data_ptr(), approximate=approximate)
    scattered = [sentinels(torch, total) for _ in range(28)]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for f in range(28):
        capi.scatter_cells_device(phi.data_ptr(), 28, f, cells.data_ptr(), ncell, scattered[f].data_ptr(), *BLOCK,
                                  status.data_ptr())
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    at = cells.cpu().numpy()
    phi_h = phi.cpu().numpy()
    for f in range(28):
        ff = helpers.bits(from_fields[f].cpu().numpy())
        assert np.array_equal(helpers.bits(phi_h[:, f]), ff[at]), f
        # whole arrays, untouched cells included: the fields form's values at the cells, the sentinel elsewhere
        want = np.full(total, SENTINEL, dtype=np.uint32)
        want[at] = ff[at]
        assert np.array_equal(helpers.bits(scattered[f].cpu().numpy()), want), f


# ---- 5. composition ----

def test_interactions_of_a_gathered_column(torch_cuda, contribs_model, block_state):
    torch = torch_cuda
    _, _, fields = block_state
    im, jm, km = BLOCK
    box = (7, 7, 4, 4, 1, km)
    buf, count, status = select_device(torch, BLOCK, box, None, None, 0.0)
    assert count == km == 8 and status == 0
    want_rows, _ = cs.gather(fields, synth.IS2D[:NFIELD], synth.PL_FEATURE, *BLOCK, buf[:count])
    rows, _ = gather_device(torch, fields, synth.IS2D[:NFIELD], synth.PL_FEATURE, BLOCK, buf[:count])
    assert np.array_equal(rows, helpers.bits(want_rows))
    d_rows = to_dev(torch, rows.view(np.float32))
    b = capi.Booster(model_buffer=contribs_model.image)
    dmat = capi.DMatrix(device_ptr=d_rows.data_ptr(), nrow=count, ncol=NFIELD, missing=synth.XX_MISS)
    out = torch.zeros((count, 28, 28), dtype=torch.float32, device="cuda")
    b.predict_interactions_device(dmat, out.data_ptr())
    torch.cuda.synchronize()
    want = b.predict_interactions(capi.DMatrix(want_rows, missing=synth.XX_MISS))
    assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(want))


def rows_as_fields(rows, grid):
    """An (im*jm*km, F) row matrix as F 3-D fields whose cell c holds row c."""
    return [rows[:, f].reshape(grid, order="F") for f in range(rows.shape[1])]


def test_a_categorical_and_a_three_group_booster_predict_on_gathered_rows(torch_cuda):
    torch = torch_cuda
    grid = (6, 5, 4)
    image, _, cat_max = catsup.make_booster(5, 6)
    X = catsup.rows(17, 120, cat_max)
    fields = rows_as_fields(X, grid)
    cells = cell_lists(50, 120, 2)["shuffled"]
    got, status = gather_device(torch, fields, [False] * 27, -1, grid, cells)
    assert status == 0 and np.array_equal(got, helpers.bits(X[cells]))
    d_rows = to_dev(torch, got.view(np.float32))
    multi, _, _ = og.make_multi(3, 6, 3, "round_robin")
    for img in (image, multi):
        b = capi.Booster(model_buffer=img)
        on_device = b.predict(capi.DMatrix(device_ptr=d_rows.data_ptr(), nrow=50, ncol=27, missing=np.nan), option_mask=1)
        on_host = b.predict(capi.DMatrix(X[cells], missing=np.nan), option_mask=1)
        assert on_device.size == (150 if img is multi else 50)
        assert np.array_equal(helpers.bits(on_device), helpers.bits(on_host))
    assert capi.Booster(model_buffer=image).num_categorical_splits() > 0


# ---- 6. Fortran ----

def test_fortran_driver(torch_cuda):
    im, jm, km = 4, 3, 6
    i, j, k = np.meshgrid(np.arange(1, im + 1), np.arange(1, jm + 1), np.arange(1, km + 1), indexing="ij")
    lat = (10 * i + j)[:, :, 0].astype(np.float32)
    pl = (1000 * k * k + 37 * i + 11 * j).astype(np.float32)
    t = (200 + i + 2 * j + 3 * k).astype(np.float32)
    alb = ((i * j)[:, :, 0].astype(np.float32) / np.float32(8))
    tropp = (9000 + 500 * i + 100 * j)[:, :, 0].astype(np.float32)
    for ic, jc in ((2, 1), (4, 3)):
        r = helpers.run_driver(DRIVER, ic, jc, timeout=120)
        assert r.returncode == 0, r.stdout
        lines = r.stdout.split("\n")
        cells = cs.select(im, jm, km, (ic, ic, jc, jc, 1, km), pl, tropp)
        rows, _ = cs.gather([lat, pl, t, alb], [True, False, False, True], 1, im, jm, km, cells)
        assert 0 < cells.size < km
        assert lines[0].split() == ["count", str(cells.size)]
        for n, c in enumerate(cells):
            got = [int(x) for x in lines[1 + n].split()]
            assert got[0] == c
            assert np.array_equal(np.array(got[1:], dtype=np.int32).view(np.uint32), helpers.bits(rows[n])), n


# ---- 7. Python ----

@pytest.mark.parametrize("what", ["contribs", "interactions"])
def test_explain_cells_is_the_five_calls(torch_cuda, contribs_model, block_state, what):
    torch = torch_cuda
    pl, tropp, fields = block_state
    im, jm, km = BLOCK
    total = im * jm * km
    box = (3, 5, 2, 3, K1, K2) if what == "contribs" else (7, 7, 4, 4, 5, 7)
    b = capi.Booster(model_buffer=contribs_model.image)
    dev_fields = [to_dev(torch, fflat(f)) for f in fields]
    d_pl, d_tropp = to_dev(torch, fflat(pl)), to_dev(torch, fflat(tropp))
    cells, out = b.explain_cells(dev_fields, synth.IS2D[:NFIELD], synth.PL_FEATURE, *BLOCK, synth.XX_MISS, box=box,
                                 a=d_pl, b=d_tropp, what=what)
    torch.cuda.synchronize()
    # the five calls
    buf, count, status = select_device(torch, BLOCK, box, pl, tropp, 0.0)
    assert count > 0 and np.array_equal(cells.cpu().numpy(), buf[:count])
    rows, _ = gather_device(torch, fields, synth.IS2D[:NFIELD], synth.PL_FEATURE, BLOCK, buf[:count])
    d_rows = to_dev(torch, rows.view(np.float32))
    dmat = capi.DMatrix(device_ptr=d_rows.data_ptr(), nrow=count, ncol=NFIELD, missing=synth.XX_MISS)
    ncol = 28 if what == "contribs" else 28 * 28
    vals = torch.zeros((count, ncol), dtype=torch.float32, device="cuda")
    if what == "contribs":
        b.predict_contribs_device(dmat, vals.data_ptr())
    else:
        b.predict_interactions_device(dmat, vals.data_ptr())
    torch.cuda.synchronize()
    assert out.shape == (ncol, total)
    want = np.full((ncol, total), np.nan, dtype=np.float32)
    want[:, buf[:count]] = vals.cpu().numpy().T
    assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(want))
    cells2, per_cell = b.explain_cells(dev_fields, synth.IS2D[:NFIELD], synth.PL_FEATURE, *BLOCK, synth.XX_MISS,
                                       cells=cells, what=what, scatter=False)
    torch.cuda.synchronize()
    assert np.array_equal(helpers.bits(per_cell.cpu().numpy()), helpers.bits(vals.cpu().numpy()))
