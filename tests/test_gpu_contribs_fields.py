"""Per-feature contributions from the MAPL fields (OHXBoosterPredictContribsFields / ...Device, csrc/contribs.hip
contribs_fields_kernel): every out[f] at levels k1..k2 bit for bit against OHXBoosterPredictContribs on the rows the
fields kernels walk, in both modes and every launch shape; the forms, the untouched levels and the NULL outputs; local
accuracy against the fields predict's margin; other feature counts, 2-D fields and no PL division; +-inf; the
refusals; buffers kept apart from a captured fields predict; and the Fortran driver's layout."""
import os

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as bs
from tests import contribs_support as cs
from tests import helpers

pytestmark = pytest.mark.gpu

C12 = synth.GRIDS["C12"]
SENTINEL = np.uint32(0x7FC0DEAD)          # a quiet NaN with a payload: nothing the kernels compute
DRIVER = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "contribs_fields_driver_hip")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def contribs_model():
    """The synthetic OH recipe at 20 trees (depth <= 18, grown on C12)."""
    return synth.make_model(num_trees=20, max_depth=18, sample_log2=16, min_leaf=2, grid=synth.GRIDS["C12"])


@pytest.fixture(scope="module")
def oh_fields():
    """The synthetic state's 27 fields on C12 L72, [i,j,k]-indexed, -999 and NaN salted into 3-D and 2-D fields."""
    _, _, fields = helpers.synth_state(C12)
    rng = np.random.default_rng(12)
    out = []
    for f in fields:
        f = np.array(f, dtype=np.float32)
        salt = rng.random(f.shape)
        f[salt < 2e-3] = np.float32(synth.XX_MISS)
        f[(salt >= 2e-3) & (salt < 4e-3)] = np.float32(np.nan)
        out.append(f)
    return out


def flat(fields):
    return [helpers.fortran_flat(f).ravel() for f in fields]


def sentinel_outputs(grid, n):
    return [np.full(grid[0] * grid[1] * grid[2], SENTINEL, dtype=np.uint32).view(np.float32) for _ in range(n)]


def gather(fields, pl_feature, k1, k2):
    """The rows the fields kernels walk, for any feature count: 2-D fields ([i,j]) broadcast over the levels, field
    pl_feature / 100 as a float32 division; rows m = i + im*(j + jm*(k-k1))."""
    im, jm = fields[0].shape[:2]
    nlev = k2 - k1 + 1
    out = np.empty((nlev, jm, im, len(fields)), dtype=np.float32)
    for f, a in enumerate(fields):
        if a.ndim == 2:
            out[..., f] = a.T[None, :, :]
        else:
            sl = a[:, :, k1 - 1:k2]
            if f == pl_feature:
                sl = (sl / np.float32(100.0)).astype(np.float32)
            out[..., f] = np.transpose(sl, (2, 1, 0))
    return out.reshape(nlev * jm * im, len(fields))


def check_against_rows(b, out, rows, grid, k1, k2, missing, approximate, ntree_limit=0, nfeat=27):
    """Every out[f] at levels k1..k2 == predict_contribs on the gathered rows, column f, bit for bit; the other
    levels keep the sentinel."""
    want = b.predict_contribs(capi.DMatrix(rows, missing=missing), approximate=approximate, ntree_limit=ntree_limit)
    plane = grid[0] * grid[1]
    lo, hi = plane * (k1 - 1), plane * k2
    for f in range(nfeat + 1):
        got = helpers.bits(out[f])
        assert np.array_equal(got[lo:hi], helpers.bits(want[:, f])), f
        assert np.all(got[:lo] == SENTINEL) and np.all(got[hi:] == SENTINEL), f


def call_host(b, fields, is2d, pl_feature, grid, k1, k2, missing, nout, **kw):
    out = sentinel_outputs(grid, nout)
    b.predict_contribs_fields(flat(fields), is2d, pl_feature, *grid, k1, k2, missing, out, **kw)
    return out


# ---- 1. the OH recipe ----

@pytest.mark.parametrize("which", ["20 trees", "100 trees"])
@pytest.mark.parametrize("approximate", [True, False])
def test_oh_recipe_against_the_rows_form(contribs_model, deep_model, oh_fields, which, approximate):
    model = contribs_model if which == "20 trees" else deep_model
    if approximate:
        k1, k2 = 20, 40
    else:
        k1, k2 = (35, 36) if which == "20 trees" else (36, 36)
    b = capi.Booster(model_buffer=model.image)
    rows = bs.engineered_rows(oh_fields, k1, k2)
    assert np.isnan(rows).any() and (rows == np.float32(synth.XX_MISS)).any()
    for ntree_limit in (0, 1, model.num_trees + 5):
        out = call_host(b, oh_fields, synth.IS2D, synth.PL_FEATURE, C12, k1, k2, synth.XX_MISS, 28,
                        approximate=approximate, ntree_limit=ntree_limit)
        check_against_rows(b, out, rows, C12, k1, k2, synth.XX_MISS, approximate, ntree_limit)


# ---- 2. launch shapes ----

@pytest.mark.parametrize("approximate", [True, False])
def test_both_sides_of_the_split_switch(contribs_model, oh_fields, approximate):
    """A one-level slab (trees split over waves) and, in approximate mode, a 20-level C48 slab (one wave per tile),
    each also with "ohx_contribs_split" = off.  Exact mode's direct side on a big slab is the two-launch test below."""
    if approximate:
        grid = synth.GRIDS["C48"]
        fields = helpers.synth_state(grid)[2]
        slabs = [(30, 30), (21, 40)]
    else:
        grid, fields, slabs = C12, oh_fields, [(30, 30)]
    plane = grid[0] * grid[1]
    shapes = [synth.contribs_plan(plane * (k2 - k1 + 1), 27, contribs_model.num_trees)[0] for k1, k2 in slabs]
    assert shapes == [True, False][:len(slabs)], shapes
    b = capi.Booster(model_buffer=contribs_model.image)
    for k1, k2 in slabs:
        rows = bs.engineered_rows(fields, k1, k2)
        for split in ("auto", "off"):
            b.set_param("ohx_contribs_split", split)
            out = call_host(b, fields, synth.IS2D, synth.PL_FEATURE, grid, k1, k2, synth.XX_MISS, 28,
                            approximate=approximate)
            check_against_rows(b, out, rows, grid, k1, k2, synth.XX_MISS, approximate)


def test_exact_direct_form_in_two_launches():
    """More than 8 192 tiles: exact mode's direct form takes two launches."""
    rng = np.random.default_rng(31)
    js, _, _ = cs.random_booster(rng, 4, 27, 5, 0.2)
    grid = (128, 128, 34)
    k1, k2 = 2, 34
    nrow = 128 * 128 * 33
    split, _, _, launches = synth.contribs_plan(nrow, 27, 4)
    assert not split and launches == 2
    fields = [cs.random_rows(rng, grid[0] * grid[1] * grid[2], 1).reshape(grid[2], grid[1], grid[0]).T
              for _ in range(27)]
    b = capi.Booster(model_buffer=js)
    out = call_host(b, fields, [False] * 27, -1, grid, k1, k2, -999.0, 28)
    check_against_rows(b, out, gather(fields, -1, k1, k2), grid, k1, k2, -999.0, False)


# ---- 3. forms and outputs ----

@pytest.mark.parametrize("approximate", [True, False])
def test_host_and_device_forms_agree_and_nulls(torch_cuda, contribs_model, oh_fields, approximate):
    torch = torch_cuda
    k1, k2 = (10, 50) if approximate else (40, 41)
    b = capi.Booster(model_buffer=contribs_model.image)
    host = call_host(b, oh_fields, synth.IS2D, synth.PL_FEATURE, C12, k1, k2, synth.XX_MISS, 28,
                     approximate=approximate)
    dev_fields = [torch.from_numpy(f.copy()).cuda() for f in flat(oh_fields)]
    n = C12[0] * C12[1] * C12[2]
    wanted = [f % 3 != 1 for f in range(28)]
    dev_out = [torch.from_numpy(np.full(n, SENTINEL, dtype=np.uint32).view(np.int32)).cuda().view(torch.float32)
               for _ in range(28)]
    b.predict_contribs_fields_device([t.data_ptr() for t in dev_fields], synth.IS2D, synth.PL_FEATURE, *C12, k1, k2,
                                     synth.XX_MISS, [t.data_ptr() if w else 0 for t, w in zip(dev_out, wanted)],
                                     approximate=approximate)
    torch.cuda.synchronize()
    for f in range(28):
        got = helpers.bits(dev_out[f].cpu().numpy())
        if wanted[f]:
            assert np.array_equal(got, helpers.bits(host[f])), f
        else:
            assert np.all(got == SENTINEL), f
    # the host form with NULL entries: those are not written, the others unchanged
    some = sentinel_outputs(C12, 28)
    b.predict_contribs_fields(flat(oh_fields), synth.IS2D, synth.PL_FEATURE, *C12, k1, k2, synth.XX_MISS,
                              [o if w else None for o, w in zip(some, wanted)], approximate=approximate)
    for f in range(28):
        assert np.array_equal(helpers.bits(some[f]), helpers.bits(host[f]) if wanted[f] else
                              np.full(n, SENTINEL, dtype=np.uint32)), f
    # only the bias
    bias_only = sentinel_outputs(C12, 1)[0]
    b.predict_contribs_fields(flat(oh_fields), synth.IS2D, synth.PL_FEATURE, *C12, k1, k2, synth.XX_MISS,
                              [None] * 27 + [bias_only], approximate=approximate)
    assert np.array_equal(helpers.bits(bias_only), helpers.bits(host[27]))


def test_empty_slab_and_all_null(contribs_model, oh_fields):
    b = capi.Booster(model_buffer=contribs_model.image)
    out = call_host(b, oh_fields, synth.IS2D, synth.PL_FEATURE, C12, 30, 29, synth.XX_MISS, 28)
    assert all(np.all(helpers.bits(o) == SENTINEL) for o in out)
    with pytest.raises(capi.OhxError, match="every entry of out is NULL"):
        b.predict_contribs_fields(flat(oh_fields), synth.IS2D, synth.PL_FEATURE, *C12, 30, 31, synth.XX_MISS,
                                  [None] * 28)


@pytest.mark.parametrize("approximate", [True, False])
def test_growing_field_count_on_one_booster(contribs_model, oh_fields, approximate):
    """The host form's per-field staging buffers grow with nfield: calls with 20, then 27, then 20 fields on ONE
    booster each match the rows form (features at or past nfield missing) bit for bit.  A staging buffer that lost its
    allocation when the list grew would alias another field's and show here."""
    k1, k2 = (25, 45) if approximate else (44, 45)
    b = capi.Booster(model_buffer=contribs_model.image)
    for nfield in (20, 27, 20, 27):
        out = call_host(b, oh_fields[:nfield], synth.IS2D[:nfield], synth.PL_FEATURE, C12, k1, k2, synth.XX_MISS, 28,
                        approximate=approximate)
        rows = np.ascontiguousarray(bs.engineered_rows(oh_fields, k1, k2)[:, :nfield])
        check_against_rows(b, out, rows, C12, k1, k2, synth.XX_MISS, approximate)


def test_fields_predict_with_growing_field_count(contribs_model, oh_fields):
    """The same growth through the fields predict's own staging buffers (they share the buffer type): after a call
    with 20 fields, a call with 27 gives what a fresh booster gives."""
    k1, k2 = 10, 60
    plane = C12[0] * C12[1]
    nrow = plane * (k2 - k1 + 1)

    def margins(b, nfield):
        oh = np.zeros(plane * C12[2], dtype=np.float32)
        margin = np.zeros(nrow, dtype=np.float32)
        b.predict_fields(flat(oh_fields[:nfield]), synth.IS2D[:nfield], synth.PL_FEATURE, *C12, k1, k2, synth.XX_MISS,
                         oh, apply_pow10=False, margin=margin)
        return margin

    b = capi.Booster(model_buffer=contribs_model.image)
    margins(b, 20)
    grown = margins(b, 27)
    fresh = margins(capi.Booster(model_buffer=contribs_model.image), 27)
    assert np.array_equal(helpers.bits(grown), helpers.bits(fresh))


# ---- 4. local accuracy ----

@pytest.mark.parametrize("approximate", [True, False])
def test_local_accuracy_against_the_fields_margin(contribs_model, oh_fields, approximate):
    k1, k2 = (5, 60) if approximate else (50, 51)
    b = capi.Booster(model_buffer=contribs_model.image)
    out = call_host(b, oh_fields, synth.IS2D, synth.PL_FEATURE, C12, k1, k2, synth.XX_MISS, 28,
                    approximate=approximate)
    plane = C12[0] * C12[1]
    nrow = plane * (k2 - k1 + 1)
    oh = np.zeros(plane * C12[2], dtype=np.float32)
    margin = np.zeros(nrow, dtype=np.float32)
    b.predict_fields(flat(oh_fields), synth.IS2D, synth.PL_FEATURE, *C12, k1, k2, synth.XX_MISS, oh,
                     apply_pow10=False, margin=margin)
    phi = np.stack([o[plane * (k1 - 1):plane * k2] for o in out], axis=1).astype(np.float64)
    err = np.abs(phi.sum(axis=1) - margin.astype(np.float64))
    bound = 1e-5 * (1.0 + np.abs(phi[:, :27]).sum(axis=1))
    assert np.all(err <= bound), float(np.max(err / bound))


# ---- 5. generality ----

@pytest.mark.parametrize("nfeat", [1, 32])
@pytest.mark.parametrize("approximate", [True, False])
def test_other_feature_counts_with_2d_fields(nfeat, approximate):
    rng = np.random.default_rng(500 + nfeat)
    js, _, _ = cs.random_booster(rng, 6, nfeat, 7, 0.25)
    grid = (16, 10, 9)
    k1, k2 = 3, 7
    is2d = [f % 3 == 2 for f in range(nfeat)] if nfeat > 1 else [False]
    fields = []
    for f in range(nfeat):
        shape = grid[:2] if is2d[f] else grid
        n = int(np.prod(shape))
        fields.append(cs.random_rows(rng, n, 1).reshape(shape[::-1]).T.copy())
    b = capi.Booster(model_buffer=js)
    for pl_feature in (-1, 0):
        for missing in (-999.0, float("nan")):
            out = call_host(b, fields, is2d, pl_feature, grid, k1, k2, missing, nfeat + 1, approximate=approximate)
            check_against_rows(b, out, gather(fields, pl_feature, k1, k2), grid, k1, k2, missing, approximate,
                               nfeat=nfeat)


@pytest.mark.parametrize("approximate", [True, False])
def test_inf_in_and_outside_the_slab(contribs_model, oh_fields, approximate):
    b = capi.Booster(model_buffer=contribs_model.image)
    k1, k2 = 30, 31
    fields = [f.copy() for f in oh_fields]
    fields[5][3, 4, 29] = np.float32(np.inf)                # level 30: inside
    with pytest.raises(capi.OhxError, match="inf"):
        call_host(b, fields, synth.IS2D, synth.PL_FEATURE, C12, k1, k2, synth.XX_MISS, 28, approximate=approximate)
    fields = [f.copy() for f in oh_fields]
    fields[5][3, 4, 40] = np.float32(-np.inf)               # level 41: outside
    fields[1][0, 0, 0] = np.float32(np.inf)                 # PL, level 1: outside
    out = call_host(b, fields, synth.IS2D, synth.PL_FEATURE, C12, k1, k2, synth.XX_MISS, 28, approximate=approximate)
    check_against_rows(b, out, bs.engineered_rows(fields, k1, k2), C12, k1, k2, synth.XX_MISS, approximate)
    # `missing` infinite: +-inf in the slab is accepted
    fields[5][3, 4, 29] = np.float32(np.inf)
    out = call_host(b, fields, synth.IS2D, synth.PL_FEATURE, C12, k1, k2, float("inf"), 28, approximate=approximate)
    check_against_rows(b, out, bs.engineered_rows(fields, k1, k2), C12, k1, k2, float("inf"), approximate)
    # and the booster is still usable after the error
    out = call_host(b, oh_fields, synth.IS2D, synth.PL_FEATURE, C12, k1, k2, synth.XX_MISS, 28, approximate=approximate)
    check_against_rows(b, out, bs.engineered_rows(oh_fields, k1, k2), C12, k1, k2, synth.XX_MISS, approximate)


# ---- 6. refusals ----

def test_refusals(torch_cuda, contribs_model, oh_fields):
    torch = torch_cuda
    ff = flat(oh_fields)
    out = sentinel_outputs(C12, 28)
    b = capi.Booster(model_buffer=contribs_model.image)

    def refused(match, *, booster=b, fields=ff, is2d=synth.IS2D, nf=None, grid=C12, k1=30, k2=31, approximate=False):
        with pytest.raises(capi.OhxError, match=match):
            booster.predict_contribs_fields(fields if nf is None else fields[:nf], is2d, synth.PL_FEATURE, *grid, k1,
                                            k2, synth.XX_MISS, out, approximate=approximate)

    refused("holds no model", booster=capi.Booster())
    refused("Number of columns does not match", fields=ff + [ff[0]], is2d=list(synth.IS2D) + [False])
    refused("im, jm, km must be positive", grid=(0, 72, 72))
    refused("need 1 <= k1", k1=0)
    refused("need 1 <= k1", k2=73)
    refused("need 1 <= k1", k1=30, k2=28)
    # no cover statistics
    js, _, _ = cs.random_booster(np.random.default_rng(3), 2, 27, 4, 0.0)
    import json
    doc = json.loads(js)
    for t in doc["learner"]["gradient_booster"]["model"]["trees"]:
        t["sum_hessian"] = [0.0] * len(t["sum_hessian"])
    refused("no cover statistics", booster=capi.Booster(model_buffer=json.dumps(doc).encode()))
    # more than 32 features
    js33, _, _ = cs.random_booster(np.random.default_rng(4), 2, 33, 3, 0.0)
    refused("at most 32 features", booster=capi.Booster(model_buffer=js33))
    # NULL pointers (through the C entry point)
    lib = capi.load_library()
    import ctypes as C
    ptrs = (C.c_void_p * 27)(*[f.ctypes.data for f in ff])
    flags = (C.c_int32 * 27)(*[1 if x else 0 for x in synth.IS2D])
    outs = (C.c_void_p * 28)(*[o.ctypes.data for o in out])
    assert lib.OHXBoosterPredictContribsFields(b.handle, None, flags, 27, 1, *C12, 30, 31, -999.0, 0, 0, outs) == -1
    assert b"NULL argument" in lib.XGBGetLastError()
    assert lib.OHXBoosterPredictContribsFields(b.handle, ptrs, None, 27, 1, *C12, 30, 31, -999.0, 0, 0, outs) == -1
    assert lib.OHXBoosterPredictContribsFields(b.handle, ptrs, flags, 27, 1, *C12, 30, 31, -999.0, 0, 0, None) == -1
    ptrs[4] = None
    assert lib.OHXBoosterPredictContribsFields(b.handle, ptrs, flags, 27, 1, *C12, 30, 31, -999.0, 0, 0, outs) == -1
    assert b"field 4 is NULL" in lib.XGBGetLastError()
    assert all(np.all(helpers.bits(o) == SENTINEL) for o in out)
    # the device form under capture: refused, nothing enqueued
    dev_fields = [torch.from_numpy(f.copy()).cuda() for f in ff]
    n = C12[0] * C12[1] * C12[2]
    dev_out = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(28)]
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="not capturable"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.predict_contribs_fields_device([t.data_ptr() for t in dev_fields], synth.IS2D, synth.PL_FEATURE, *C12,
                                             30, 31, synth.XX_MISS, [t.data_ptr() for t in dev_out],
                                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0.0 for t in dev_out)


# ---- 7. buffers kept apart ----

def test_buffers_stay_apart_from_a_captured_fields_predict(torch_cuda, deep_model):
    torch = torch_cuda
    grid = (48, 36, 72)
    pl, tropp, fields = helpers.synth_state(grid)
    k1, k2 = 20, 60
    dev = [torch.from_numpy(helpers.fortran_flat(f).ravel().copy()).cuda() for f in fields]
    n = grid[0] * grid[1] * grid[2]
    oh = torch.zeros(n, dtype=torch.float32, device="cuda")
    b = capi.Booster(model_buffer=deep_model.image)
    s = torch.cuda.Stream()

    def call(stream):
        b.predict_fields_device([t.data_ptr() for t in dev], synth.IS2D, synth.PL_FEATURE, *grid, k1, k2,
                                synth.XX_MISS, oh.data_ptr(), stream=stream)

    with torch.cuda.stream(s):
        call(s.cuda_stream)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    oh.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    first = oh.cpu().numpy().copy()
    # a bigger host-form contributions call on the same booster in between
    _, _, big = helpers.synth_state(synth.GRIDS["C48"])
    out = sentinel_outputs(synth.GRIDS["C48"], 28)
    b.predict_contribs_fields(flat(big), synth.IS2D, synth.PL_FEATURE, *synth.GRIDS["C48"], 1, 72, synth.XX_MISS, out,
                              approximate=True)
    oh.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    b.check()
    assert np.array_equal(helpers.bits(oh.cpu().numpy()), helpers.bits(first))
    assert np.any(first != 0)


# ---- 8. Fortran ----

@pytest.mark.parametrize("approximate", [1, 0])
def test_fortran_driver_layout(tmp_path, contribs_model, approximate):
    assert os.path.exists(DRIVER), DRIVER
    grid = (24, 20, 72)
    pl, tropp, fields = helpers.synth_state(grid)
    state = tmp_path / "state.bin"
    helpers.write_state_file(str(state), pl, tropp, fields, False)
    model = tmp_path / "oh.model"
    model.write_bytes(bytes(contribs_model.image))
    k1, k2 = (10, 40) if approximate else (33, 34)
    res = tmp_path / "out.bin"
    r = helpers.run_driver(DRIVER, state, model, res, k1, k2, approximate)
    assert r.returncode == 0, r.stdout
    raw = open(res, "rb").read()
    assert np.frombuffer(raw, dtype="<i4", count=1)[0] == 0
    c = np.frombuffer(raw, dtype="<f4", offset=4).reshape(28, -1)
    b = capi.Booster(model_buffer=contribs_model.image)
    out = [np.zeros(grid[0] * grid[1] * grid[2], dtype=np.float32) for _ in range(28)]
    b.predict_contribs_fields(flat(fields), synth.IS2D, synth.PL_FEATURE, *grid, k1, k2, synth.XX_MISS, out,
                              approximate=bool(approximate))
    for f in range(28):
        assert np.array_equal(helpers.bits(c[f]), helpers.bits(out[f])), f
