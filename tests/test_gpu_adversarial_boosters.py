"""The shipped walk kernels on adversarial boosters (tests/booster_shapes.py): root leaves, stumps, full trees of 4 and 5
steps, chains to depth 30, both phases mixed in one group of four, ties on every threshold, +-inf as the missing marker.
Every case is compared with the C oracle bit for bit, and every margin case first asks the library which kernels the
predict launches (Booster.kernel_symbols_for), so that it cannot pass on another path than the one it is about."""
import functools

import numpy as np
import pytest

from oracle import xgb_oracle as O
from quickchem_amd import capi, oh_predict, synth
from tests import booster_shapes as S
from tests import helpers

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 5, 10, 135)
MISSING = (-999.0, float("nan"), float("inf"), float("-inf"))
KERNELS = ("wide", "packed1", "packed2", "packed4", "super1", "super2", "super3", "super4", "ring")
RESIDENCY = 256 * 16 * 64          # rows the chip holds at once: CUs x waves of a ring block x 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@functools.lru_cache(maxsize=None)
def booster(ntree):
    js, trees = S.make_booster(1000 + ntree, ntree)
    return js, synth.convert_model(js, "binary"), trees


@functools.lru_cache(maxsize=None)
def rows(ntree, n, missing):
    _, _, trees = booster(ntree)
    if n <= 8192:
        return S.rows_for(ntree, trees, n, missing)
    # big batches: a 64 Ki-row block (random rows, then tie rows) repeated, so the tie rows fill whole waves
    block = S.rows_for(ntree + 7, trees, 65536, missing)
    return np.ascontiguousarray(np.resize(block, (n, S.NFEAT)))


@functools.lru_cache(maxsize=None)
def want(ntree, n, missing, ntree_limit=0):
    return helpers.oracle_predict(booster(ntree)[1], rows(ntree, n, missing), missing, ntree_limit=ntree_limit)


def same(got, ref, what):
    assert np.array_equal(helpers.bits(got), helpers.bits(ref)), (what, int(np.sum(helpers.bits(got) != helpers.bits(ref))))


def check_kernel(b, d, kernel, split, ntree, small):
    """The launch is the kernel the case is about: its family, and whether the trees are split over waves."""
    sym = b.kernel_symbols_for(d)
    if kernel == "wide":
        assert sym == "predict_rows_direct_kernel<false>", sym
        return sym
    is_super = kernel.startswith("super") or kernel == "ring"
    splits = split == "auto" and is_super and ntree >= 8 and small
    if kernel == "ring" and not splits:
        assert sym.startswith("predict_rows_ring_kernel + "), sym
    else:
        chains = 2 if kernel == "ring" else int(kernel[-1])
        assert sym.startswith(f"predict_rows_tile_kernel<{2 if is_super else 1},{chains},"), sym
    assert ("combine_leaves_kernel" in sym) == splits, sym
    return sym


def predict_checked(b, x, missing, kernel, split, ntree, what, ref, grid=None):
    d = capi.DMatrix(x, missing=missing)
    if grid is not None:
        d.set_grid(*grid)
    check_kernel(b, d, kernel, split, ntree, small=len(x) <= 8192)
    same(b.predict(d), ref, what)
    if kernel == "ring":
        assert b.ring_reruns() == 0, what          # the ring walked it, not the tile kernel behind it
    d.free()


@pytest.mark.parametrize("ntree", COUNTS)
def test_every_kernel_on_adversarial_boosters(ntree):
    """Every ohx_kernel, trees split over waves (auto, on these 3000 rows) and one wave per tile (off), every marker."""
    js, _, _ = booster(ntree)
    for kernel in KERNELS:
        b = capi.Booster(model_buffer=js)
        b.set_param("ohx_kernel", kernel)
        for split in ("auto", "off"):
            b.set_param("ohx_tree_split", split)
            for missing in MISSING:
                predict_checked(b, rows(ntree, 3000, missing), missing, kernel, split, ntree, (kernel, split, missing),
                                want(ntree, 3000, missing))
        b.free()


@pytest.mark.parametrize("missing", MISSING)
def test_ring_batch_sizes(missing):
    """The ring kernel from one row to more than two residencies of the chip (the last one ragged), and the same small
    batches the split way."""
    ntree = 135
    js, _, _ = booster(ntree)
    for n, splits in ((1, ("off",)), (63, ("auto", "off")), (65, ("auto", "off")), (RESIDENCY // 2 + 4099, ("off",)),
                      (2 * RESIDENCY + 4097, ("auto",))):
        b = capi.Booster(model_buffer=js)
        b.set_param("ohx_kernel", "ring")
        for split in splits:
            b.set_param("ohx_tree_split", split)
            predict_checked(b, rows(ntree, n, missing), missing, "ring", split, ntree, (n, split, missing),
                            want(ntree, n, missing))
        b.free()


@pytest.mark.parametrize("ntree", (10, 135))
def test_ring_knobs(ntree):
    """ohx_ring_rounds 0 (one launch) and 1 (a launch per residency), rows with missing values walked in the ring or
    left to the second launch, on rows said to lie on a grid (rounds apply to those)."""
    js, _, _ = booster(ntree)
    n = 37 * 53 * 60
    for missing in MISSING:
        x, ref = rows(ntree, n, missing), want(ntree, n, missing)
        for rounds in (0, 1):
            for defer in ("on", "off"):
                b = capi.Booster(model_buffer=js)
                b.set_param("ohx_kernel", "ring")
                b.set_param("ohx_tree_split", "off")
                b.set_param("ohx_ring_rounds", rounds)
                b.set_param("ohx_defer_missing", defer)
                d = capi.DMatrix(x, missing=missing)
                d.set_grid(37, 53, 0)
                sym = check_kernel(b, d, "ring", "off", ntree, small=False)
                assert ("rows with missing values" in sym) == (defer == "on"), sym
                same(b.predict(d), ref, (rounds, defer, missing))
                assert b.ring_reruns() == 0
                d.free()
                b.free()


def test_ring_clustered_shuffled_rows():
    """Shuffled rows through the clustering pass's permutation into the ring."""
    ntree = 135
    js, _, _ = booster(ntree)
    for missing in (-999.0, float("-inf")):
        x = rows(ntree, 3000, missing)
        perm = np.random.default_rng(5).permutation(len(x))
        x, ref = np.ascontiguousarray(x[perm]), want(ntree, 3000, missing)[perm]
        b = capi.Booster(model_buffer=js)
        for k, v in (("ohx_kernel", "ring"), ("ohx_tree_split", "off"), ("ohx_cluster", "on"), ("ohx_cluster_trees", 4),
                     ("ohx_cluster_steps", 3)):
            b.set_param(k, v)
        d = capi.DMatrix(x, missing=missing)
        d.set_grid(0, 0, 0)
        check_kernel(b, d, "ring", "off", ntree, small=False)
        same(b.predict(d), ref, ("cluster", missing))
        assert b.ring_reruns() == 0
        d.free()
        b.free()


@pytest.mark.parametrize("ntree", (10, 135))
def test_tree_tops_both_ways(ntree):
    js, _, _ = booster(ntree)
    for kernel in ("super1", "super2", "super3", "super4"):
        for tops in ("on", "off"):
            b = capi.Booster(model_buffer=js)
            for k, v in (("ohx_kernel", kernel), ("ohx_tree_split", "off"), ("ohx_tree_tops", tops)):
                b.set_param(k, v)
            for missing in (-999.0, float("nan"), float("inf")):
                d = capi.DMatrix(rows(ntree, 3000, missing), missing=missing)
                sym = check_kernel(b, d, kernel, "off", ntree, small=True)
                assert sym.endswith("true>" if tops == "on" else "false>"), sym
                same(b.predict(d), want(ntree, 3000, missing), (kernel, tops, missing))
                d.free()
            b.free()


def test_ntree_limit():
    ntree = 135
    js, _, _ = booster(ntree)
    for kernel, split in (("ring", "off"), ("super2", "auto"), ("super3", "off"), ("packed2", "off")):
        b = capi.Booster(model_buffer=js)
        b.set_param("ohx_kernel", kernel)
        b.set_param("ohx_tree_split", split)
        for missing in (-999.0, float("-inf")):
            d = capi.DMatrix(rows(ntree, 3000, missing), missing=missing)
            check_kernel(b, d, kernel, split, ntree, small=True)
            for limit in (1, 2, 3, 5, 129):
                same(b.predict(d, ntree_limit=limit), want(ntree, 3000, missing, limit), (kernel, split, missing, limit))
            d.free()
        b.free()


@pytest.mark.parametrize("ntree", COUNTS)
def test_leaf_indices(ntree):
    """option_mask = 16 against the numpy oracle's pred_leaf (kernel_symbols_for names margin predicts only)."""
    js, _, _ = booster(ntree)
    model = O.load_model(js)
    for missing in MISSING:
        x = rows(ntree, 3000, missing)
        b = capi.Booster(model_buffer=js)
        b.set_param("ohx_kernel", "ring")
        leaves = b.predict(capi.DMatrix(x, missing=missing), option_mask=16).reshape(len(x), -1)
        assert np.array_equal(leaves, O.predict(model, x, missing=missing, pred_leaf=True)), missing
        b.free()


def test_device_form_through_the_ring(torch_cuda):
    torch = torch_cuda
    ntree = 135
    js, _, _ = booster(ntree)
    n = RESIDENCY // 2 + 4099
    for missing in (float("nan"), float("-inf")):
        x = torch.from_numpy(rows(ntree, n, missing)).to("cuda:0")
        b = capi.Booster(model_buffer=js)
        b.set_param("ohx_kernel", "ring")
        b.set_param("ohx_tree_split", "off")
        d = capi.DMatrix(device_ptr=x.data_ptr(), nrow=n, ncol=S.NFEAT, missing=missing)
        check_kernel(b, d, "ring", "off", ntree, small=False)
        out = torch.zeros(n, dtype=torch.float32, device="cuda:0")
        b.predict_device(d, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        b.check()
        assert b.ring_reruns() == 0
        same(out.cpu().numpy(), want(ntree, n, missing), ("device", missing))
        d.free()
        b.free()


# ---- the fused path: thresholds on the engineered values ----

def salted_state(grid, seed):
    pl, tropp, fields = helpers.synth_state(grid)
    rng = np.random.default_rng(seed)
    fields = [f.copy() for f in fields]
    for f in fields[2:]:                                  # LAT and PL stay (the slab is made from PL)
        mask = rng.random(f.shape) < 2e-3
        f[mask] = np.where(rng.random(int(mask.sum())) < 0.5, np.float32(synth.XX_MISS), np.float32(np.nan))
    return pl, tropp, fields


def fields_model(fields, k1, k2, seed, ntree=40):
    eng = S.engineered_rows(fields, k1, k2)
    eng = np.where(eng == np.float32(synth.XX_MISS), np.float32(np.nan), eng)
    pick = np.random.default_rng(seed).choice(len(eng), min(len(eng), 200000), replace=False)
    js, _ = S.fields_booster(seed, ntree, eng[pick])
    return js, synth.convert_model(js, "binary")


@pytest.mark.parametrize("grid,cases", [((12, 72, 72), (("ring", "auto"), ("ring", "off"), ("super2", "auto"))),
                                        ((144, 96, 80), (("ring", "on"), ("ring", "off")))])
def test_fused_fields_on_engineered_thresholds(torch_cuda, grid, cases):
    """OHPredictor's fused call on a slab with -999.0 and NaN in its fields, on a booster whose thresholds ARE the slab's
    engineered values (PL / 100, the 2-D broadcast) or their float32 neighbours: a feature one ulp off moves a leaf.
    The small slab: trees split over waves, or not; the big one: predict_fields_ring_kernel, missing rows deferred or
    walked in the ring.  Margins bit for bit."""
    pl, tropp, fields = salted_state(grid, 29)
    k1, k2 = O.k_slab(pl, tropp, True, 4000.0)
    js, binary = fields_model(fields, k1, k2, grid[0])
    oh_ref, margin_ref, k1, k2 = helpers.oracle_predict_oh(binary, pl, tropp, fields, True)
    nrow = grid[0] * grid[1] * (k2 - k1 + 1)
    big = nrow >= 2 * RESIDENCY
    assert big == (grid[0] == 144), nrow
    for kernel, knob in cases:
        p = oh_predict.OHPredictor()
        p.xx_bst = capi.Booster(model_buffer=js)
        p.xx_bst.set_param("ohx_kernel", kernel)
        if big:
            p.xx_bst.set_param("ohx_defer_missing", knob)
        else:
            p.xx_bst.set_param("ohx_tree_split", knob)
        sym = p.xx_bst.kernel_symbol(27)
        assert sym == "predict_rows_ring_kernel" if kernel == "ring" else sym.startswith("predict_rows_tile_kernel<2,2,"), sym
        if big:
            assert p.xx_bst.fields_kernel_symbol(nrow) == "predict_fields_ring_kernel"
        p.first_time = False
        oh = np.zeros(grid, dtype=np.float32)
        margins = []
        assert p.predict_OH_with_XGB("unused", *grid, True, 4000.0, pl, tropp, oh_predict.OHBoostInputData(fields), oh,
                                     mode="fused", margin_out=margins) == 0
        same(margins[0], margin_ref, (kernel, knob))
        if kernel == "ring":
            assert p.xx_bst.ring_reruns() == 0
        assert np.all(oh[:, :, :k1 - 1] == 0)
        assert helpers.ulp_diff(oh[:, :, k1 - 1:], oh_ref[:, :, k1 - 1:]).max() <= 2


# ---- OH Run1 ----

def oracle_run1(image, st, **kw):
    b = capi.Booster(model_buffer=image, lib=helpers.oracle_lib())
    out = b.run1(st, **kw)
    b.free()
    return out


@pytest.mark.parametrize("grid", [(48, 24, 72), (144, 200, 72)])
def test_run1_on_engineered_thresholds(grid):
    """OHXBoosterRun1 with a booster whose thresholds are Run1's own engineered features (numpy oracle's restatement)
    and their neighbours, on a rank-sized block and on a slab that takes the ring: what test_run1_gpu_vs_oracle asserts."""
    st = helpers.run1_state(grid, seed=grid[1])
    leaf = S.booster_json([S.make_tree(np.random.default_rng(0), "leaf", None)], 0.0)
    eng = O.run1(O.load_model(leaf), st, True)
    rows = S.engineered_rows(eng["fields"], eng["k1"], eng["k2"])
    pick = np.random.default_rng(1).choice(len(rows), min(len(rows), 200000), replace=False)
    js, _ = S.fields_booster(grid[0], 40, rows[pick])
    binary = synth.convert_model(js, "binary")
    want_ = oracle_run1(binary, st, dynamic_k_range=True)
    b = capi.Booster(model_buffer=js)
    b.set_param("ohx_kernel", "ring")
    assert b.kernel_symbol(27) == "predict_rows_ring_kernel"
    nrow = grid[0] * grid[1] * (want_["k2"] - want_["k1"] + 1)
    assert (nrow >= 2 * RESIDENCY) == (grid[0] == 144), nrow
    got = b.run1(st, dynamic_k_range=True)
    assert b.ring_reruns() == 0
    assert (got["k1"], got["k2"]) == (want_["k1"], want_["k2"])
    assert np.array_equal(helpers.bits(got["ndwet"]), helpers.bits(want_["ndwet"]))
    k1 = got["k1"]
    assert np.all(got["oh_boost"][:, :, :k1 - 1] == 0)
    assert helpers.ulp_diff(got["oh_boost"][:, :, k1 - 1:], want_["oh_boost"][:, :, k1 - 1:]).max() <= 2
    pl = (st["ple_mod"][:, :, :-1] + st["ple_mod"][:, :, 1:]) * np.float32(0.5)
    above = ~(pl > st["tropp_mod"][:, :, None])
    assert np.array_equal(helpers.bits(got["oh"][above]), helpers.bits(want_["oh"][above]))
    assert helpers.ulp_diff(got["oh"][~above], want_["oh"][~above]).max() <= 3
