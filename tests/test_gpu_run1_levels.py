"""OH Run1's arithmetic around the walk - feature_pointwise_kernel, the column-sum kernels, k_slab_kernel and
post_process_kernel (kernels.hip) - at every level count a GEOS configuration might use and on every path of
launch_feature_prep:

  wave kernel      (a rank-sized plane, or a piece beside a walk) and km <= 128: a lane per level, two above 64
  reg<72>          a plane over 8 192 columns at km = 72
  LDS kernel       everything else: four waves per block up to 160 levels, fewer above (the LDS of a CU holds 160 KiB),
                   one from 321 levels to the limit of 640

The engineered features (the DIAG dumps) are held bit for bit to oracle/xgb_oracle.py:run1_features, NDWET and the slab
bit for bit to the C oracle, OH_boost and OH to it within the tolerances of test_run1.py::test_run1_gpu_vs_oracle."""
import numpy as np
import pytest

from oracle import xgb_oracle as O
from quickchem_amd import capi
from tests import helpers

pytestmark = pytest.mark.gpu

f32 = np.float32
SMALL = (13, 7)            # 91 columns: no multiple of a wave or of a block's four
BIG = (96, 90)             # 8 640 columns: over the 8 192 where the wave kernel stops
KMS = [1, 2, 7, 8, 9, 63, 64, 65, 71, 73, 91, 127, 128, 129, 132, 137, 159, 160, 161, 181]
FEATURES = capi.RUN1_DIAG_3D + ["diag_strato3"]


def oracle_run1(model, st, **kw):
    b = capi.Booster(model_buffer=model.image, lib=helpers.oracle_lib())
    try:
        return b.run1(st, **kw)
    finally:
        b.free()


def gpu_run1(model, st, params=(), **kw):
    b = capi.Booster(model_buffer=model.image)
    try:
        for k, v in params:
            b.set_param(k, v)
        out = b.run1(st, **kw)
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    finally:
        b.free()


def same_bits(got, want, what):
    """Bit for bit; NaN by position (a NaN's payload is the hardware's business)."""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(helpers.bits(got[~nan]), helpers.bits(want[~nan])), what


def pl_mod(st):
    ple = st["ple_mod"]
    return ((ple[:, :, :-1] + ple[:, :, 1:]) * f32(0.5)).astype(f32)


def check_against_references(got, want, st):
    """got: the GPU's run1 with want_diag; want: the C oracle's."""
    with np.errstate(all="ignore"):
        feat = O.run1_features(st)
    for name in FEATURES:
        same_bits(got[name], feat[name], name)
    assert (got["k1"], got["k2"]) == (want["k1"], want["k2"])
    same_bits(got["ndwet"], want["ndwet"], "ndwet")
    k1 = got["k1"]
    assert np.all(got["oh_boost"][:, :, :k1 - 1] == 0)
    assert helpers.ulp_diff(got["oh_boost"][:, :, k1 - 1:], want["oh_boost"][:, :, k1 - 1:]).max(initial=0) <= 2
    above = ~(pl_mod(st) > st["tropp_mod"][:, :, None])
    assert np.array_equal(helpers.bits(got["oh"][above]), helpers.bits(want["oh"][above]))
    assert helpers.ulp_diff(got["oh"][~above], want["oh"][~above]).max(initial=0) <= 3


def run_and_check(model, st, dynamic, tropp_min=4000.0):
    kw = dict(dynamic_k_range=dynamic, tropp_min=tropp_min, want_diag=True)
    want = oracle_run1(model, st, **kw)
    got = gpu_run1(model, st, **kw)
    check_against_references(got, want, st)
    return got, want


# ---- the level sweep on a small plane: the wave kernel up to 128 levels, the LDS kernel above

@pytest.mark.parametrize("km", KMS)
def test_run1_levels_small_plane(small_model, km):
    st = helpers.run1_state(SMALL + (km,), seed=km)
    run_and_check(small_model, st, dynamic=True)


@pytest.mark.parametrize("km", [1, 64, 65, 137, 181])
def test_run1_levels_small_plane_static(small_model, km):
    st = helpers.run1_state(SMALL + (km,), seed=100 + km)
    run_and_check(small_model, st, dynamic=False)


# ---- the plane-size switch at 8 192 columns, and big planes off 72 levels

@pytest.mark.parametrize("km", [72, 91])
@pytest.mark.parametrize("plane", [(128, 64), (43, 191)])
def test_run1_plane_size_switch(small_model, plane, km):
    st = helpers.run1_state(plane + (km,), seed=plane[0] + km)
    run_and_check(small_model, st, dynamic=True)


@pytest.mark.parametrize("km", [91, 137, 160, 181])
def test_run1_big_plane_off_72(small_model, km):
    st = helpers.run1_state(BIG + (km,), seed=km)
    run_and_check(small_model, st, dynamic=True)


@pytest.mark.parametrize("km", [91, 137, 181])
def test_run1_pieces_off_72(deep_model, km):
    """ohx_run1_pieces = 3: the features of the third piece are computed beside the first piece's walk (beside_a_walk);
    every output is the one-piece output, which is the references'."""
    st = helpers.run1_state(BIG + (km,), seed=7 * km)
    kw = dict(dynamic_k_range=True, want_diag=True)
    want = oracle_run1(deep_model, st, **kw)
    one, many = (gpu_run1(deep_model, st, params=(("ohx_kernel", "ring"), ("ohx_run1_pieces", n)), **kw) for n in (1, 3))
    for name, v in one.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(helpers.bits(many[name]), helpers.bits(v)), name
        else:
            assert many[name] == v, name
    check_against_references(many, want, st)


# ---- values on the boundaries of the slab count and the tropopause mask

def boundary_state(km, seed, all_and_none=False):
    """Every column's TROPP is its own PL_MOD at one of its levels (q_mod = 0 there), so `PL > TROPP` is false exactly
    there in k_slab_kernel and post_process_kernel.  all_and_none: also a column whose every level counts (k1 = 1) and
    one where none does."""
    st = helpers.run1_state(SMALL + (km,), seed=seed)
    rng = np.random.default_rng(seed)
    pl = pl_mod(st)
    tropp, q = st["tropp_mod"].copy(), st["q_mod"].copy()
    for i in range(SMALL[0]):
        for j in range(SMALL[1]):
            k = int(rng.integers(km))
            tropp[i, j] = pl[i, j, k]
            q[i, j, k] = 0.0
    if all_and_none:
        tropp[0, 0] = f32(0.5)                      # under the top level's PL: every level counts
        tropp[1, 0] = f32(2.0e5)                    # over the surface: none does
    st["tropp_mod"], st["q_mod"] = tropp, q
    return st


@pytest.mark.parametrize("km", [1, 8, 65, 137, 181])
def test_run1_slab_and_mask_on_the_boundary(small_model, km):
    st = boundary_state(km, seed=km)
    got, _ = run_and_check(small_model, st, dynamic=True)
    pl = pl_mod(st)
    assert got["k1"] == km - int((pl > st["tropp_mod"][:, :, None]).sum(axis=2).max()) + 1
    on = pl == st["tropp_mod"][:, :, None]
    assert on.sum() == SMALL[0] * SMALL[1]
    want_oh = ((st["default_oh"] * got["ndwet"]).astype(f32) * f32(1e-6)).astype(f32)
    assert np.array_equal(helpers.bits(got["oh"][on]), helpers.bits(want_oh[on]))
    both = boundary_state(km, seed=km, all_and_none=True)
    got, _ = run_and_check(small_model, both, dynamic=True)
    assert got["k1"] == 1


@pytest.mark.parametrize("km", [8, 65, 137, 181])
def test_run1_static_on_the_boundary(small_model, km):
    """Static slab: TROPP_MIN equal to a PL_MOD of the plane (`PL > TROPP_MIN` false there); a column with
    TROPP == TROPP_MIN is refused as the reference refuses it, its float neighbour above is not."""
    st = helpers.run1_state(SMALL + (km,), seed=200 + km)
    pl = pl_mod(st)
    low = pl[(pl < 8000) & (pl > 100)]
    tropp_min = float(low.max())
    got, _ = run_and_check(small_model, st, dynamic=False, tropp_min=tropp_min)
    assert got["k1"] == km - int((pl > f32(tropp_min)).sum(axis=2).max()) + 1
    st["tropp_mod"] = st["tropp_mod"].copy()
    st["tropp_mod"][5, 3] = f32(tropp_min)
    for make in (lambda: oracle_run1(small_model, st, dynamic_k_range=False, tropp_min=tropp_min),
                 lambda: gpu_run1(small_model, st, dynamic_k_range=False, tropp_min=tropp_min)):
        with pytest.raises(capi.OhxError, match="Minimum tropopause pressure"):
            make()
    st["tropp_mod"][5, 3] = np.nextafter(f32(tropp_min), f32(np.inf))
    run_and_check(small_model, st, dynamic=False, tropp_min=tropp_min)


@pytest.mark.parametrize("km", [1, 65, 181])
def test_post_process_alone_on_the_boundary(km):
    st = boundary_state(km, seed=300 + km, all_and_none=True)
    oh_ml = (st["default_oh"] * f32(7.0)).astype(f32)
    args = (st["ple_mod"], st["t_mod"], st["q_mod"], st["tropp_mod"], st["default_oh"], oh_ml)
    got = capi.oh_post_process(*args)
    want = capi.oh_post_process(*args, lib=helpers.oracle_lib())
    for g, w, name in zip(got, want, ("oh", "ndwet")):
        same_bits(g, w, name)


# ---- NaN and overflow in the column sums

@pytest.mark.parametrize("km", [65, 137, 181])
def test_run1_nan_in_a_column_sum(small_model, km):
    """A NaN in TAUCLW at level k0 of one column: NaN in exactly SUM(x(1:k)) for k >= k0 and SUM(x(k:km)) for k <= k0."""
    st = helpers.run1_state(SMALL + (km,), seed=400 + km)
    k0 = km // 2
    st["tauclw"] = st["tauclw"].copy()
    st["tauclw"][4, 2, k0] = np.nan
    got, _ = run_and_check(small_model, st, dynamic=True)
    want_up, want_dn = np.zeros((*SMALL, km), bool), np.zeros((*SMALL, km), bool)
    want_up[4, 2, k0:] = True
    want_dn[4, 2, :k0 + 1] = True
    assert np.array_equal(np.isnan(got["diag_tauclwup"]), want_up)
    assert np.array_equal(np.isnan(got["diag_tauclwdn"]), want_dn)
    for name in FEATURES:
        if name not in ("diag_tauclwup", "diag_tauclwdn"):
            assert not np.isnan(got[name]).any(), name


@pytest.mark.parametrize("km", [65, 181])
def test_run1_overflow_in_a_column_sum(small_model, km):
    """Finite TAUCLW whose sums reach +inf.  Inside the slab, or above it where SUM(x(1:k)) carries the inf down into
    it: refused ("Input data contains `inf` or `nan`") by the GPU exactly as by the oracle.  Only in a SUM(x(k:km)) of
    a level above the slab: no refusal on either side, and the inf is in that DIAG dump."""
    st = helpers.run1_state(SMALL + (km,), seed=500 + km)
    k1 = oracle_run1(small_model, st, dynamic_k_range=True)["k1"]
    assert k1 >= 4                                  # levels 1..3 (1-based) lie above the slab
    big = f32(3.0e38)
    for levels, values in (((km - 2, km - 1), (big, big)), ((0, 1), (big, big))):
        bad = dict(st, tauclw=st["tauclw"].copy())
        bad["tauclw"][6, 1, list(levels)] = values
        for make in (lambda: oracle_run1(small_model, bad, dynamic_k_range=True),
                     lambda: gpu_run1(small_model, bad, dynamic_k_range=True)):
            with pytest.raises(capi.OhxError, match="inf"):
                make()
    # -big + big + big: SUM(x(2:km)) overflows, SUM(x(1:km)), SUM(x(3:km)) and every SUM(x(1:k)) do not
    ok = dict(st, tauclw=st["tauclw"].copy())
    ok["tauclw"][6, 1, :3] = (-big, big, big)
    got, _ = run_and_check(small_model, ok, dynamic=True)
    dn = got["diag_tauclwdn"]
    assert np.isposinf(dn[6, 1, 1]) and np.isinf(dn).sum() == 1
    assert np.isfinite(got["diag_tauclwup"]).all()


# ---- the level limit (include/ohxgb.h): the LDS kernel with one wave per block at 640 levels, refused above

def test_run1_at_the_level_limit_and_over_it(small_model):
    st = helpers.run1_state((5, 3, 640), seed=640)
    run_and_check(small_model, st, dynamic=True)
    over = helpers.run1_state((5, 3, 641), seed=641)
    b = capi.Booster(model_buffer=small_model.image)
    try:
        with pytest.raises(capi.OhxError, match="km = 641 levels; the limit is 640"):
            b.run1(over, dynamic_k_range=True)
        # refused before anything was enqueued: the same booster's next tick is the oracle's
        got = b.run1(st, dynamic_k_range=True, want_diag=True)
        check_against_references(got, oracle_run1(small_model, st, dynamic_k_range=True, want_diag=True), st)
    finally:
        b.free()
