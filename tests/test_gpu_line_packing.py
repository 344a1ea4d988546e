"""The walk kernels on every placement of the super-node groups ("ohx_super_pack" 0..3, csrc/flatten.hpp kSuperPack*):
the shapes of tests/line_packing_support.py - a wrong group number, a misplaced filler or a tree base off by one group
sends some row of them to another leaf - and eight random depth-12 trees, through the ring rows kernel, the ring
fields kernel, the tile kernel with tree tops and the deferred rows' second launch, forced the way
tests/test_gpu_adversarial_boosters.py forces them.  Margins against the C oracle bit for bit; no ring re-run.

Rows: 16 x 16 x 8 gridcells with the grid named, and 4 096 rows without.  The ring FIELDS kernel only takes slabs that
fill the chip twice (kernels.hip plan_fields: 256 CUs x 16 waves x 64 x 2 = 524 288 gridcells), so its case runs on the
smallest slab of the adversarial tests that does, 144 x 96 x 80; the small grid's fused call goes the tile way."""
import functools

import numpy as np
import pytest

from oracle import xgb_oracle as O
from quickchem_amd import capi, oh_predict, synth
from tests import booster_shapes as S
from tests import helpers
from tests import line_packing_support as L

pytestmark = pytest.mark.gpu

NAMES = ("stump", "left", "right", "complete", "parity", "phases", "cap", "random")
MISSING = float(synth.XX_MISS)
GRID = (16, 16, 8)
SLAB = (144, 96, 80)


def same(got, ref, what):
    assert np.array_equal(helpers.bits(got), helpers.bits(ref)), (what, int(np.sum(helpers.bits(got) != helpers.bits(ref))))


@functools.lru_cache(maxsize=None)
def row_world():
    """The rows (gridcells of the synthetic state; the flat batch half tie rows led down the boosters' trees, and a copy
    with 1e-3 of its values missing), the boosters with thresholds on them, the oracle's margins - computed once."""
    rng = np.random.default_rng(3)
    on_grid = synth.rows_cpu(GRID, 0, GRID[0] * GRID[1] * GRID[2])
    flat = synth.rows_cpu((64, 64, 72), 64 * 64 * 20, 2048)
    forests = L.make_forests(np.concatenate([on_grid, flat]), which=NAMES)
    out = {}
    for name, (js, trees) in forests.items():
        binary = synth.convert_model(js, "binary")
        x = np.ascontiguousarray(np.concatenate([flat, S.tie_rows(rng, trees, 2048, base=flat)]), dtype=np.float32)
        holes = x.copy()
        holes[rng.random(holes.shape) < 1e-3] = np.float32(MISSING)
        batches = {"grid": on_grid, "flat": x, "holes": holes}
        out[name] = (js, {k: (v, helpers.oracle_predict(binary, v, MISSING)) for k, v in batches.items()})
    return out


@functools.lru_cache(maxsize=None)
def slab_world():
    """The 144 x 96 x 80 state with -999.0 and NaN salted into its fields, boosters with thresholds on the slab's
    engineered rows, the oracle's fused margins - computed once."""
    pl, tropp, fields = helpers.synth_state(SLAB)
    rng = np.random.default_rng(29)
    fields = [f.copy() for f in fields]
    for f in fields[2:]:
        mask = rng.random(f.shape) < 1e-3
        f[mask] = np.where(rng.random(int(mask.sum())) < 0.5, np.float32(MISSING), np.float32(np.nan))
    k1, k2 = O.k_slab(pl, tropp, True, 4000.0)
    eng = S.engineered_rows(fields, k1, k2)
    eng = np.where(eng == np.float32(MISSING), np.float32(np.nan), eng)
    pick = rng.choice(len(eng), 20000, replace=False)
    out = {}
    for name, (js, _) in L.make_forests(eng[pick], seed=7, which=NAMES).items():
        _, margin, k1, k2 = helpers.oracle_predict_oh(synth.convert_model(js, "binary"), pl, tropp, fields, True)
        out[name] = (js, margin)
    return (pl, tropp, fields, SLAB[0] * SLAB[1] * (k2 - k1 + 1)), out


def booster(js, pack, **params):
    b = capi.Booster(model_buffer=js)
    b.set_param("ohx_super_pack", pack)
    for k, v in params.items():
        b.set_param(k, v)
    return b


def predict(b, x, ref, what, grid, expect):
    d = capi.DMatrix(x, missing=MISSING)
    if grid:
        d.set_grid(GRID[0], GRID[1], 0)
    sym = b.kernel_symbols_for(d)
    expect(sym)
    same(b.predict(d), ref, what)
    assert b.ring_reruns() == 0, what
    d.free()


@pytest.mark.parametrize("pack", L.PACKS)
def test_ring_rows_kernel(pack):
    for name, (js, batches) in row_world().items():
        b = booster(js, pack, ohx_kernel="ring", ohx_tree_split="off", ohx_defer_missing="off")

        def ring(sym):
            assert sym.startswith("predict_rows_ring_kernel + ") and "rows with missing values" not in sym, sym
        for key in ("grid", "flat", "holes"):
            predict(b, *batches[key], (name, pack, key), key == "grid", ring)
        b.free()


@pytest.mark.parametrize("pack", L.PACKS)
def test_tile_kernel_with_tree_tops(pack):
    for name, (js, batches) in row_world().items():
        b = booster(js, pack, ohx_kernel="super2", ohx_tree_split="off", ohx_tree_tops="on")

        def tops(sym):
            assert sym.startswith("predict_rows_tile_kernel<2,2,") and sym.endswith("true>"), sym
        for key in ("grid", "flat", "holes"):
            predict(b, *batches[key], (name, pack, key), key == "grid", tops)
        b.free()


@pytest.mark.parametrize("pack", L.PACKS)
def test_deferred_second_launch(pack):
    """1e-3 of the values missing: those rows are left to the second launch behind the ring's"""
    for name, (js, batches) in row_world().items():
        b = booster(js, pack, ohx_kernel="ring", ohx_tree_split="off", ohx_defer_missing="on")

        def deferred(sym):
            assert sym.startswith("predict_rows_ring_kernel + ") and "rows with missing values" in sym, sym
        x, ref = batches["holes"]
        assert 40 < np.count_nonzero((x == np.float32(MISSING)).any(axis=1)) < len(x) // 2
        predict(b, x, ref, (name, pack), False, deferred)
        b.free()


@pytest.mark.parametrize("pack", L.PACKS)
def test_ring_fields_kernel(pack):
    (pl, tropp, fields, nrow), boosters = slab_world()
    for name, (js, margin_ref) in boosters.items():
        p = oh_predict.OHPredictor()
        p.xx_bst = booster(js, pack, ohx_kernel="ring")
        assert p.xx_bst.fields_kernel_symbol(nrow) == "predict_fields_ring_kernel", nrow
        p.first_time = False
        oh = np.zeros(SLAB, dtype=np.float32)
        margins = []
        assert p.predict_OH_with_XGB("unused", *SLAB, True, 4000.0, pl, tropp, oh_predict.OHBoostInputData(fields), oh,
                                     mode="fused", margin_out=margins) == 0
        same(margins[0], margin_ref, (name, pack))
        assert p.xx_bst.ring_reruns() == 0
        p.xx_bst.free()
