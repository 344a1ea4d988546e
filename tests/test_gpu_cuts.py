"""Quantile cuts from rows in HBM (csrc/cuts.hip) through DMatrix.quantile_cuts.  Pointers and values are compared with
the numpy restatement of the header (tests/grow_support.quantile_cuts) on x[::row_step], which calls nothing; no returned
cut may be a negative zero.  The column kinds are those of tests/cuts_support.py."""
import ctypes as C

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import cuts_support as CS
from tests import helpers
from tests import visits_support as V

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def device_matrix(torch, x, missing, stream=None):
    """-> (DMatrix that borrows HBM, the tensor that owns it)."""
    if stream is not None:
        with torch.cuda.stream(stream):
            t = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    else:
        t = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
        torch.cuda.synchronize()
    return capi.DMatrix(device_ptr=t.data_ptr(), nrow=x.shape[0], ncol=x.shape[1], missing=missing), t


def run(torch, x, missing, max_bins, row_step=1, what=""):
    d, t = device_matrix(torch, x, missing)
    got = d.quantile_cuts(row_step, max_bins)
    d.free()
    CS.same_cuts(got, x[::row_step], missing, max_bins, what)
    return got


def wide(x, ncol):
    """ncol columns: the kinds repeated, each repeat scaled so that no two columns are equal."""
    reps = -(-ncol // x.shape[1])
    return np.ascontiguousarray(np.concatenate([x * np.float32(1 + r) for r in range(reps)], axis=1)[:, :ncol])


@pytest.mark.parametrize("missing", [NAN, -999.0, float("inf")])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_every_column_kind_at_the_small_row_counts(torch_cuda, n, missing):
    for max_bins in (2, 64, 255):
        x = CS.columns(n, max_bins, missing)
        d, t = device_matrix(torch_cuda, x, missing)
        for step in (1, 3, 64, n + 1):
            CS.same_cuts(d.quantile_cuts(step, max_bins), x[::step], missing, max_bins, (n, max_bins, missing, step))
        d.free()


@pytest.mark.parametrize("ncol", [1, 3, 27, 128])
def test_column_counts(torch_cuda, ncol):
    """At 128 columns pass 1 takes several column groups and the prefix stage fills its LDS."""
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    p = synth.cuts_plan(4097, 1, ncol, cus)
    assert p["col_groups1"] == -(-ncol // 10) and p["lds_bytes"] == ncol * 255 * 4
    for max_bins in (64, 255):
        base = CS.columns(4097, max_bins, -999.0)
        if ncol >= base.shape[1]:
            run(torch_cuda, wide(base, ncol), -999.0, max_bins, 1, (ncol, max_bins))
        else:
            for k in range(0, base.shape[1], ncol):        # every kind, ncol columns at a time
                run(torch_cuda, np.ascontiguousarray(base[:, k:k + ncol]), -999.0, max_bins, 1, (ncol, max_bins, k))


def test_more_rows_than_two_trips_of_each_kernels_loop(torch_cuda):
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    full = synth.cuts_plan(1 << 30, 1, 3, cus)
    n = 2 * full["block_rows"] * max(full["blocks1"], full["blocks"]) + 1
    p = synth.cuts_plan(n, 1, 3, cus)
    assert n > 2 * p["block_rows"] * p["blocks1"] and n > 2 * p["block_rows"] * p["blocks"]
    rng = np.random.default_rng(5)
    x = np.empty((n, 3), dtype=np.float32)
    x[:, 0] = rng.normal(0, 1, n)
    x[:, 1] = (np.uint32(0x3F800000) + rng.integers(0, 1024, n).astype(np.uint32)).view(np.float32)
    x[:, 2] = np.where(rng.random(n) < 0.6, 0.0, rng.normal(0, 1, n))
    x[rng.random(n) < 0.01, 0] = np.nan
    got = run(torch_cuda, x, NAN, 255, 1, "past the launch caps")
    assert np.diff(got[0].astype(np.int64)).tolist()[0] == 254


def test_one_add_per_wave_and_an_add_per_lane(torch_cuda):
    """A sampled row is a lane.  Column 0 is constant inside every run of 64 sampled rows and differs between runs,
    column 1 is constant throughout: a wave makes one add.  Column 2 alternates two values lane by lane: every lane adds.
    Column 3 is constant except in one lane of every wave."""
    step, ns = 3, 64 * 50 + 17
    n = (ns - 1) * step + 2
    rng = np.random.default_rng(8)
    x = rng.normal(0, 1, (n, 4)).astype(np.float32)      # the rows between the sampled ones are never looked at
    i = np.arange(ns)
    x[::step, 0] = (i // 64) * 0.5
    x[::step, 1] = 7.25
    x[::step, 2] = np.where(i % 2 == 0, -1.5, 2.5)
    x[::step, 3] = np.where(i % 64 == 13, i.astype(np.float32), 4.0)
    for max_bins in (2, 16, 255):
        got = run(torch_cuda, x, NAN, max_bins, step, max_bins)
        assert got[0][2] - got[0][1] == 0 and got[1][int(got[0][2]):int(got[0][3])].tolist() == [2.5]


def test_both_forms_a_stream_the_row_order_the_grid_and_a_second_call_change_no_bit(torch_cuda):
    torch = torch_cuda
    n = 1200
    x = CS.columns(n, 32, -999.0)
    x[~np.isfinite(x) & ~np.isnan(x)] = 0.5          # (the host form refuses +-inf in its rows)
    first = None
    perm = np.random.default_rng(1).permutation(n)
    xp = np.ascontiguousarray(x[perm])
    for what, rws, grid, device in (("plain", x, None, False), ("permuted", xp, None, False),
                                    ("grid said", x, (12, 10, 0), False), ("device form", x, None, True),
                                    ("device form, grid said, permuted", xp, (12, 10, 0), True)):
        s = torch.cuda.Stream() if device else None
        if device:
            d, t = device_matrix(torch, rws, -999.0, s)
        else:
            d = capi.DMatrix(rws, missing=-999.0)
        if grid is not None:
            d.set_grid(*grid)
        for call in range(2):
            ptr, vals = d.quantile_cuts(1, 32, stream=s.cuda_stream if device else None)
            if first is None:
                first = (ptr, vals)
                CS.same_cuts(first, x, -999.0, 32)
            assert np.array_equal(ptr, first[0]), (what, call)
            assert np.array_equal(helpers.bits(vals), helpers.bits(first[1])), (what, call)
        d.free()


def raw(lib, d, row_step, max_bins, ptr, vals, cap, needed, stream=None):
    rc = lib.OHXDMatrixQuantileCuts(d.handle if d is not None else None, row_step, max_bins,
                                    ptr.ctypes.data if ptr is not None else None,
                                    vals.ctypes.data if vals is not None else None, cap,
                                    C.byref(needed) if needed is not None else None, stream)
    return rc, lib.XGBGetLastError().decode()


def test_a_cap_one_too_small_then_exact(torch_cuda):
    lib = capi.load_library()
    x = np.arange(20, dtype=np.float32).reshape(10, 2)
    d, t = device_matrix(torch_cuda, x, NAN)
    ptr = np.zeros(3, dtype=np.uint64)
    vals = np.full(18, -7.0, dtype=np.float32)
    needed = C.c_uint64()
    rc, msg = raw(lib, d, 1, 255, ptr, vals, 17, needed)
    assert rc == -1 and needed.value == 18 and "18 cut values are needed" in msg and "holds 17" in msg, msg
    assert vals[17] == -7.0, "a value was written past cap"
    rc, msg = raw(lib, d, 1, 255, ptr, vals, 18, needed)
    assert rc == 0 and needed.value == 18 and ptr.tolist() == [0, 9, 18], msg
    CS.same_cuts((ptr, vals), x, NAN, 255)
    # cap = 0 with no values asks for the count alone
    rc, msg = raw(lib, d, 1, 255, ptr, None, 0, needed)
    assert rc == -1 and needed.value == 18
    d.free()


def test_every_refusal_is_followed_by_a_valid_call(torch_cuda):
    torch = torch_cuda
    lib = capi.load_library()
    x = CS.columns(300, 16, NAN)
    d, t = device_matrix(torch, x, NAN)
    ptr = np.full(x.shape[1] + 1, 77, dtype=np.uint64)
    vals = np.full(x.shape[1] * 254, -7.0, dtype=np.float32)
    needed = C.c_uint64(12345)

    def refused(part, **kw):
        a = {"d": d, "row_step": 1, "max_bins": 16, "ptr": ptr, "vals": vals, "cap": vals.size, "needed": needed}
        a.update(kw)
        rc, msg = raw(lib, a["d"], a["row_step"], a["max_bins"], a["ptr"], a["vals"], a["cap"], a["needed"], a.get("stream"))
        assert rc == -1 and part in msg, (part, msg)
        assert np.all(ptr == 77) and np.all(vals == -7.0) and needed.value == 12345, ("a refused call wrote", part)
        CS.same_cuts(d.quantile_cuts(1, 16), x, NAN, 16, "after " + part)

    gone = capi.DMatrix(device_ptr=t.data_ptr(), nrow=4, ncol=2, missing=NAN)
    handle = C.c_void_p(gone.handle.value)
    gone.free()
    gone.handle = handle
    refused("DMatrix handle is invalid", d=gone)
    gone.handle = C.c_void_p()
    refused("DMatrix handle is invalid", d=None)
    refused("NULL output argument", ptr=None)
    refused("NULL output argument", needed=None)
    refused("cut_values is NULL", vals=None)
    for mb in (1, 0, 256, -3):
        refused("max_bins must be in 2..255", max_bins=mb)
    refused("row_step must be >= 1", row_step=0)
    many = (1 << 31) + 1
    over = capi.DMatrix(device_ptr=t.data_ptr(), nrow=many, ncol=2, missing=NAN)
    refused("at most 2^31 rows", d=over)
    over.free()
    # more counters than the card holds: 2^22 columns x 255 x 1024 x 4 bytes
    huge = capi.DMatrix(device_ptr=t.data_ptr(), nrow=1, ncol=1 << 22, missing=NAN)
    big_ptr = np.full((1 << 22) + 1, 77, dtype=np.uint64)
    rc, msg = raw(lib, huge, 1, 16, big_ptr, vals, vals.size, needed)
    assert rc == -1 and "bytes cannot be allocated" in msg, msg
    assert np.all(big_ptr == 77) and needed.value == 12345
    huge.free()
    CS.same_cuts(d.quantile_cuts(1, 16), x, NAN, 16, "after the allocation")
    # a stream that is being captured
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="stream capture"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            d.quantile_cuts(1, 16, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        CS.same_cuts(d.quantile_cuts(1, 16, stream=s.cuda_stream), x, NAN, 16, "after the capture")
    d.free()


def test_no_rows(torch_cuda):
    t = torch_cuda.zeros((64, 3), dtype=torch_cuda.float32, device="cuda")
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=0, ncol=3, missing=-999.0)
    ptr, vals = d.quantile_cuts(1, 255)
    assert ptr.tolist() == [0, 0, 0, 0] and vals.size == 0
    ptr, vals = d.quantile_cuts(7, 2, pad_to=5)
    assert ptr.tolist() == [0] * 6
    d.free()


def test_boost_trees_saves_the_same_model_with_these_cuts(torch_cuda, tmp_path):
    """End to end, on data without zeros: the cuts made on the device grow byte for byte the model that
    capi.quantile_cuts(x[::step]) grows.  The matrix has fewer columns than the booster has features."""
    js = V.random_booster(9003, 3, 3, max_depth=4, p_leaf=0.1)
    n, step = 3000, 3
    rng = np.random.default_rng(21)
    x = rng.normal(0, 1, (n, 2)).astype(np.float32)
    x[:, 1] = rng.integers(1, 6, n)
    x[rng.random(x.shape) < 0.05] = np.nan
    x[rng.random(x.shape) < 0.02] = -999.0
    assert not np.any(x == 0)
    d = capi.DMatrix(x, missing=-999.0)
    b = capi.Booster(model_buffer=js)
    margin = b.predict(d, option_mask=1).copy()
    b.free()
    y = (margin + np.where(np.nan_to_num(x[:, 0], nan=0.5) > 0.3, 1.0, -0.5) + rng.normal(0, 0.3, n)).astype(np.float32)
    host = capi.quantile_cuts(x[::step], -999.0, 64)
    host = (np.concatenate([host[0], host[0][-1:]]), host[1])
    dev = d.quantile_cuts(step, 64, pad_to=3)
    assert np.array_equal(dev[0], host[0]) and np.array_equal(helpers.bits(dev[1]), helpers.bits(host[1]))
    images = []
    for k, cuts in enumerate((host, dev)):
        b = capi.Booster(model_buffer=js)
        assert b.boost_trees(d, y, cuts, rounds=2, max_depth=4) > 2
        path = str(tmp_path / f"m{k}.json")
        b.save_model(path)
        images.append(open(path, "rb").read())
        b.free()
    d.free()
    assert images[0] == images[1]
