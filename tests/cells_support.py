"""Selected gridcells restated in numpy, from the text of include/ohxgb.h (OHXSelectCells, OHXGatherCells,
OHXScatterCells) and not from the C++, and the same again as plain Python loops (what tests/test_cells_cpu.py holds the
numpy against).  Arrays are [i,j(,k)]-indexed, 0-based; boxes are 1-based and inclusive, as the C ABI takes them.  A
cell index is c = i + im * (j + jm * k) for 0-based i, j, k."""
import numpy as np

OUT_OF_RANGE, NOT_ASCENDING, OVER_CAP = 1, 2, 4


def whole(im, jm, km):
    return (1, im, 1, jm, 1, km)


def _as3d(x, im, jm, km):
    x = np.asarray(x, dtype=np.float32)
    return np.broadcast_to(x[:, :, None], (im, jm, km)) if x.ndim == 2 else x


def select(im, jm, km, box, a=None, b=None, b0=0.0):
    """The cells of the box with a > b as float32 (b None: the scalar b0; a None: every cell; NaN selects nothing), in
    cell-index order."""
    i1, i2, j1, j2, k1, k2 = box
    inside = np.zeros((im, jm, km), dtype=bool)
    inside[i1 - 1:i2, j1 - 1:j2, k1 - 1:k2] = True
    if a is not None:
        rhs = np.float32(b0) if b is None else _as3d(b, im, jm, km)
        with np.errstate(invalid="ignore"):
            inside &= _as3d(a, im, jm, km) > rhs
    return np.flatnonzero(inside.ravel(order="F")).astype(np.int64)


def gather(fields, is2d, pl_feature, im, jm, km, cells):
    """rows[n][f] = field f at cell cells[n] (2-D fields at its (i,j)), field pl_feature / 100 in float32; a row whose
    cell is out of range is NaN.  -> (rows, status)."""
    cells = np.asarray(cells, dtype=np.int64)
    total, plane = im * jm * km, im * jm
    ok = (cells >= 0) & (cells < total)
    at = np.where(ok, cells, 0)
    rows = np.empty((cells.size, len(fields)), dtype=np.float32)
    for f, field in enumerate(fields):
        flat = np.asarray(field, dtype=np.float32).ravel(order="F")
        v = flat[at % plane] if is2d[f] else flat[at]
        if f == pl_feature:
            with np.errstate(invalid="ignore"):
                v = v / np.float32(100)
        rows[:, f] = np.where(ok, v, np.float32(np.nan))
    return rows, (OUT_OF_RANGE if not ok.all() else 0)


def scatter(values, col, cells, out_flat, total):
    """out_flat[cells[n]] = values[n, col] for every n whose cell is in range and above every entry in front of it
    (for a list with a single descent: above its predecessor).  -> (the new array, status)."""
    values = np.asarray(values, dtype=np.float32)
    values = values.reshape(len(values), -1) if values.size else values.reshape(0, 1)
    cells = np.asarray(cells, dtype=np.int64)
    out = np.array(out_flat, dtype=np.float32, copy=True)
    if cells.size == 0:
        return out, 0
    lowest = np.iinfo(np.int64).min
    front = np.concatenate([[lowest], np.maximum.accumulate(cells)[:-1]])
    above = cells > front
    ok = (cells >= 0) & (cells < total)
    write = above & ok
    out[cells[write]] = values[write, col]
    return out, (0 if ok.all() else OUT_OF_RANGE) | (0 if above.all() else NOT_ASCENDING)


# ---- the same with loops ----

def select_loops(im, jm, km, box, a=None, b=None, b0=0.0):
    i1, i2, j1, j2, k1, k2 = box
    cells = []
    for k in range(k1, k2 + 1):
        for j in range(j1, j2 + 1):
            for i in range(i1, i2 + 1):
                if a is not None:
                    a = np.asarray(a)
                    av = np.float32(a[i - 1, j - 1] if a.ndim == 2 else a[i - 1, j - 1, k - 1])
                    if b is None:
                        bv = np.float32(b0)
                    else:
                        b = np.asarray(b)
                        bv = np.float32(b[i - 1, j - 1] if b.ndim == 2 else b[i - 1, j - 1, k - 1])
                    if not av > bv:
                        continue
                cells.append((i - 1) + im * ((j - 1) + jm * (k - 1)))
    return np.array(cells, dtype=np.int64)


def gather_loops(fields, is2d, pl_feature, im, jm, km, cells):
    rows = np.empty((len(cells), len(fields)), dtype=np.float32)
    status = 0
    for n, c in enumerate(cells):
        c = int(c)
        if c < 0 or c >= im * jm * km:
            rows[n, :] = np.nan
            status |= OUT_OF_RANGE
            continue
        i, j, k = c % im, (c // im) % jm, c // (im * jm)
        for f, field in enumerate(fields):
            v = np.float32(field[i, j] if is2d[f] else field[i, j, k])
            if f == pl_feature:
                with np.errstate(invalid="ignore"):
                    v = np.float32(v / np.float32(100))
            rows[n, f] = v
    return rows, status


def scatter_loops(values, col, cells, out_flat, total):
    values = np.asarray(values, dtype=np.float32)
    values = values.reshape(len(values), -1) if values.size else values.reshape(0, 1)
    out = np.array(out_flat, dtype=np.float32, copy=True)
    status = 0
    top = None
    for n, c in enumerate(cells):
        c = int(c)
        above = top is None or c > top
        top = c if top is None else max(top, c)
        if not above:
            status |= NOT_ASCENDING
        if c < 0 or c >= total:
            status |= OUT_OF_RANGE
            continue
        if above:
            out[c] = values[n, col]
    return out, status
