"""The leaf refit on the GPU (csrc/refit.hip).  Leaf values and base_weights are compared bit for bit.

Expected leaves never come from the code under test: tests/refit_support.py restates OHXBoosterRefitLeaves in numpy
from the text of include/ohxgb.h, with a tree walk of its own.  What the library holds after a call is read through
XGBoosterSaveModel (JSON), a path already held to its own tests."""
import ctypes as C
import functools

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import helpers
from tests import refit_support as R
from tests import visits_support as V
from tests.test_random_forests import random_rows

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 4097)
UNVISITED = {"keep": 0, "zero": 1}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@functools.lru_cache(maxsize=None)
def adversarial(ntree=10):
    """Every kind of tests/booster_shapes.py at ntree = 10; 1, 2 and 5 trees are SMALL_PLANS too."""
    js, trees = S.make_booster(8000 + ntree, ntree)
    return js, trees


@functools.lru_cache(maxsize=None)
def rows_for(ntree, n, missing):
    return S.rows_for(n * 5 + ntree, adversarial(ntree)[1], n, missing)


def labels_for(seed, n, scale=1.0):
    return np.random.default_rng(seed).normal(0, scale, n).astype(np.float32)


def held(b, tmp_path, name="held.json"):
    """(value, base_weight) per tree as the booster holds them, and the JSON image."""
    path = str(tmp_path / name)
    b.save_model(path)
    image = open(path, "rb").read()
    return R.leaves_of(image), image


def same_leaves(got, want, what=""):
    (gv, gw), (wv, ww) = got, want
    assert len(gv) == len(wv)
    for t in range(len(wv)):
        bad = np.flatnonzero(helpers.bits(gv[t]) != helpers.bits(wv[t]))
        assert bad.size == 0, (what, "value", t, bad[:6], gv[t][bad[:6]], wv[t][bad[:6]])
        bad = np.flatnonzero(helpers.bits(gw[t]) != helpers.bits(ww[t]))
        assert bad.size == 0, (what, "base_weight", t, bad[:6], gw[t][bad[:6]], ww[t][bad[:6]])


def check(tmp_path, js, x, missing, y, eta=1.0, lam=1.0, unvisited="keep", what=""):
    want = R.refit(js, x, missing, y, eta, lam, UNVISITED[unvisited])
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=missing)
    n = b.refit_leaves(d, y, eta=eta, reg_lambda=lam, unvisited=unvisited)
    got, _ = held(b, tmp_path)
    d.free()
    b.free()
    assert n == want["leaves_refit"], (what, n, want["leaves_refit"])
    same_leaves(got, (want["value"], want["base_weight"]), what)
    return want


# ---- new leaves against the restatement ----

@pytest.mark.parametrize("missing", [-999.0, float("nan")], ids=["missing -999", "missing NaN"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_leaves_equal_the_restatement_on_every_kind_of_tree(torch_cuda, tmp_path, n, missing):
    """All KINDS, tie rows (rows exactly on a threshold and one step either side), NaN and -999 in the rows."""
    js, _ = adversarial()
    assert {k for k in S.SMALL_PLANS[10]} == set(S.KINDS)
    x = rows_for(10, n, missing)
    if n >= 4097:
        assert np.isnan(x).any() and (x == -999.0).any()
    want = check(tmp_path, js, x, missing, labels_for(n, n), eta=0.3, what=f"{n} rows")
    assert want["leaves_refit"] >= 10


@pytest.mark.parametrize("ntree", (1, 2, 5))
@pytest.mark.parametrize("eta,lam", [(1.0, 0.0), (0.3, 1.0)])
def test_one_two_and_five_trees(torch_cuda, tmp_path, ntree, eta, lam):
    js, _ = adversarial(ntree)
    x = rows_for(ntree, 1000, -999.0)
    check(tmp_path, js, x, -999.0, labels_for(ntree, 1000), eta=eta, lam=lam, what=f"{ntree} trees")


@pytest.mark.parametrize("ncol", (1, 20))
def test_fewer_columns_than_features(torch_cuda, tmp_path, ncol):
    js, _ = adversarial()
    x = np.ascontiguousarray(rows_for(10, 4097, -999.0)[:1000, :ncol])
    check(tmp_path, js, x, -999.0, labels_for(ncol, 1000), what=f"{ncol} columns")


@pytest.mark.parametrize("nfeat,staged", [(100, True), (300, False)], ids=["100 features", "tiles that do not fit LDS"])
def test_other_feature_counts(torch_cuda, tmp_path, nfeat, staged):
    js = V.random_booster(8200 + nfeat, 4, nfeat, max_depth=8, p_leaf=0.15)
    assert synth.refit_plan(1000, nfeat, 4)["stage"] == staged
    rng = np.random.default_rng(nfeat)
    x = random_rows(rng, 1000, nfeat)
    x[rng.random(x.shape) < 0.02] = -999.0
    check(tmp_path, js, x, -999.0, labels_for(nfeat, 1000), what=f"{nfeat} features")
    check(tmp_path, js, np.ascontiguousarray(x[:, :nfeat - 3]), -999.0, labels_for(nfeat, 1000),
          what="three columns short")


def test_more_rows_than_two_trips_of_each_kernels_loop(torch_cuda, tmp_path):
    """A block strides over its rows.  The trips come from the plan the library exports: blocks x 256 rows for the
    leaf-id walk and for the accumulate pass; more than twice the larger, and no multiple of 64.  A root-leaf tree
    takes every row's add on ONE address."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = synth.refit_plan(1 << 30, 27, 2, cus)
    trip_ids, trip_accum = full["ids_blocks"] * full["block_rows"], full["accum_blocks"] * full["block_rows"]
    assert full["ids_blocks"] == cus * full["ids_blocks_per_cu"] and full["accum_blocks"] == cus * full["accum_blocks_per_cu"]
    n = 2 * max(trip_ids, trip_accum) + 77
    p = synth.refit_plan(n, 27, 2, cus)
    assert n % 64 != 0 and n > 2 * p["ids_blocks"] * p["block_rows"] and n > 2 * p["accum_blocks"] * p["block_rows"]
    js, _ = adversarial(2)
    assert [len(t["left_children"]) for t in V.doc_trees(js)][0] == 1, "tree 0 is a root leaf"
    rng = np.random.default_rng(5)
    x = rng.normal(0, 2, (n, 27)).astype(np.float32)
    x[rng.random(x.shape) < 0.01] = np.nan
    check(tmp_path, js, x, float("nan"), labels_for(6, n), eta=0.5, what="past the launch caps")


# ---- sign and cancellation ----

def test_negative_sums_exact_cancellation_one_row_per_leaf_and_the_edge_of_the_range(torch_cuda, tmp_path):
    js = R.stump(0.0, base=0.0)
    edge = float(np.nextafter(np.float32(256.0), np.float32(0.0)))
    # left (x0 < 0): g = -y = -1.5, -0.25, 1.0 -> G < 0; right: g = 1.5, -1.5 -> G == 0 exactly
    x = np.array([[-1, 0, 0], [-2, 0, 0], [-3, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float32)
    y = np.array([1.5, 0.25, -1.0, -1.5, 1.5], dtype=np.float32)
    want = check(tmp_path, js, x, float("nan"), y, eta=1.0, lam=0.0, what="cancellation")
    assert want["G"][0].tolist() == [0, -(3 << 22), 0] and want["H"][0].tolist() == [0, 3, 2]
    assert want["value"][0][1] == np.float32(0.25) and want["value"][0][2] == 0.0
    # one row per leaf, each just inside |g| < 256, of either sign
    x = np.array([[-1, 0, 0], [1, 0, 0]], dtype=np.float32)
    y = np.array([edge, -edge], dtype=np.float32)
    want = check(tmp_path, js, x, float("nan"), y, eta=1.0, lam=0.0, what="one row per leaf at the edge")
    assert want["value"][0].tolist() == [0.0, edge, -edge] and want["leaves_refit"] == 2
    assert want["max_abs_grad"] == edge
    # many rows at the edge on one leaf: |G| is 4097 x (2^32 - 2^8)
    x = np.full((4097, 3), -1.0, dtype=np.float32)
    want = check(tmp_path, js, x, float("nan"), np.full(4097, -edge, dtype=np.float32), eta=1.0, lam=1.0, what="4097 rows at the edge")
    assert int(want["G"][0][1]) == 4097 * ((1 << 32) - (1 << 8))


def test_a_stump_is_within_the_derived_bound_of_the_float64_mean(torch_cuda, tmp_path):
    """eta = 1, lambda = 0: each leaf within 2^-24 * (1 + |m|) of m, the float64 mean of -(base - y) over its rows
    (2^-25 from the fixed point plus one float32 rounding; tests/refit_support.py stump_bound_ratio)."""
    rng = np.random.default_rng(77)
    worst = 0.0
    for case, (n, scale) in enumerate(((1, 1.0), (65, 1e-3), (333, 1.0), (1000, 100.0), (4097, 10.0))):
        base = float(rng.normal(0, scale))
        js = R.stump(rng.normal(0, 1), base=base)
        x = rng.normal(0, 1, (n, 3)).astype(np.float32)
        y = np.clip(rng.normal(0, scale, n) + rng.normal(0, scale), base - 250.0, base + 250.0).astype(np.float32)
        b = capi.Booster(model_buffer=js)
        d = capi.DMatrix(x, missing=float("nan"))
        b.refit_leaves(d, y, eta=1.0, reg_lambda=0.0)
        (value, _), _ = held(b, tmp_path)
        ratio = R.stump_bound_ratio(js, x, y, value[0])
        print(f"case {case}: {n} rows, scale {scale}: |leaf - m| / bound = {ratio:.3f}")
        worst = max(worst, ratio)
        d.free()
        b.free()
    assert worst <= 1.0, worst


# ---- independence ----

def test_the_order_of_the_rows_the_form_and_the_grid_change_no_bit(torch_cuda, tmp_path):
    torch = torch_cuda
    js, _ = adversarial()
    n = 1200
    x = rows_for(10, 4097, -999.0)[:n]
    y = labels_for(3, n)
    want = R.refit(js, x, -999.0, y, 0.3, 1.0, 0)
    ref = (want["value"], want["base_weight"])
    perm = np.random.default_rng(1).permutation(n)
    xp, yp = np.ascontiguousarray(x[perm]), np.ascontiguousarray(y[perm])
    assert R.refit(js, xp, -999.0, yp, 0.3, 1.0, 0)["leaves_refit"] == want["leaves_refit"]
    for what, rows, labels, grid, device in (("plain", x, y, None, False), ("permuted", xp, yp, None, False),
                                             ("grid said", x, y, (12, 10, 0), False),
                                             ("a shard inside a level", x[:1000], y[:1000], (12, 10, 2 * 120 + 37), False),
                                             ("device form", x, y, None, True),
                                             ("device form, grid said", x, y, (12, 10, 0), True)):
        b = capi.Booster(model_buffer=js)
        if device:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                tx = torch.from_numpy(rows).to("cuda")
                ty = torch.from_numpy(labels).to("cuda")
            s.synchronize()
            d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=len(rows), ncol=27, missing=-999.0)
        else:
            d = capi.DMatrix(rows, missing=-999.0)
        if grid is not None:
            d.set_grid(*grid)
        if device:
            got_n = b.refit_leaves_device(d, ty.data_ptr(), len(labels), eta=0.3, stream=s.cuda_stream)
        else:
            got_n = b.refit_leaves(d, labels, eta=0.3)
        got, _ = held(b, tmp_path)
        if len(rows) == n:
            assert got_n == want["leaves_refit"]
            same_leaves(got, ref, what)
        else:
            shard = R.refit(js, rows, -999.0, labels, 0.3, 1.0, 0)
            same_leaves(got, (shard["value"], shard["base_weight"]), what)
        d.free()
        b.free()


# ---- after a refit ----

def explain(b, d):
    return [b.predict_contribs(d), b.predict_contribs(d, approximate=True)]


def test_after_a_refit_everything_equals_a_booster_loaded_with_the_expected_leaves(torch_cuda, tmp_path):
    js, trees = S.contribs_booster(8105, 10)
    n = 4097
    x = S.rows_for(31, trees, n, -999.0)
    y = labels_for(9, n)
    want = R.refit(js, x, -999.0, y, 0.5, 1.0, 0)
    other = capi.Booster(model_buffer=R.with_leaves(js, want["value"], want["base_weight"]))
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=-999.0)
    # the device forms, the contributions state and the visit counters exist, and hold the OLD leaves
    dx = capi.DMatrix(x[:96], missing=-999.0)
    before = b.predict(d, option_mask=1)
    explained_before = explain(b, dx)
    b.count_visits(d)
    counts_before, seen_before = b.visit_counts()
    assert b.refit_leaves(d, y, eta=0.5) == want["leaves_refit"]
    after = b.predict(d, option_mask=1)
    assert not np.array_equal(helpers.bits(before), helpers.bits(after)), "the refit changed nothing"
    # the margin a predict makes is the sum the refit itself ran on
    assert np.array_equal(helpers.bits(after), helpers.bits(want["pred"]))
    for kernel, split in (("auto", "auto"), ("wide", "auto"), ("ring", "off")):
        for bb in (b, other):
            bb.set_param("ohx_kernel", kernel)
            bb.set_param("ohx_tree_split", split)
        sym = b.kernel_symbols_for(d)
        if kernel == "ring":
            assert sym.startswith("predict_rows_ring_kernel"), sym
        if kernel == "wide":
            assert sym == "predict_rows_direct_kernel<false>", sym
        got, ref = b.predict(d, option_mask=1), other.predict(d, option_mask=1)
        assert np.array_equal(helpers.bits(got), helpers.bits(ref)), kernel
        assert np.array_equal(helpers.bits(got), helpers.bits(want["pred"])), kernel
    assert np.array_equal(b.predict(d, option_mask=16), other.predict(d, option_mask=16))
    for g, r, o, name in zip(explain(b, dx), explain(other, dx), explained_before, ("exact", "approximate")):
        assert g.shape == r.shape and np.array_equal(helpers.bits(g), helpers.bits(r)), name
        assert not np.array_equal(helpers.bits(g), helpers.bits(o)), name
    # the visit state holds no leaf value: kept with its counters
    counts_after, seen_after = b.visit_counts()
    assert seen_after == seen_before == n
    V.assert_same_counts(counts_after, counts_before, "the visit counters")
    # the new leaves are held by all three file formats, and nothing else moved
    for ext in ("json", "ubj", "bin"):
        path = str(tmp_path / f"refit.{ext}")
        b.save_model(path)
        again = capi.Booster(model_file=path)
        got, image = held(again, tmp_path, f"back_{ext}.json")
        same_leaves(got, (want["value"], want["base_weight"]), ext)
        for t_old, t_new in zip(V.doc_trees(js), V.doc_trees(image)):
            for key in ("left_children", "right_children", "split_indices", "default_left", "sum_hessian", "loss_changes"):
                assert t_old[key] == t_new[key], (ext, key)
        assert np.array_equal(helpers.bits(again.predict(d, option_mask=1)), helpers.bits(want["pred"])), ext
        again.free()
    # a second refit starts from the refit leaves
    twice = R.refit(R.with_leaves(js, want["value"], want["base_weight"]), x, -999.0, y, 0.5, 1.0, 0)
    b.refit_leaves(d, y, eta=0.5)
    same_leaves(held(b, tmp_path)[0], (twice["value"], twice["base_weight"]), "a second refit")
    dx.free()
    d.free()


# ---- the walk the refit shares with the visit counts ----

SHARED_MISSING = -999.0


@functools.lru_cache(maxsize=None)
def shared_walk(ntree=3, depth=4):
    """The smallest case that still takes every path of the shared walk: 5 features (the 4-wide row loads have a tail),
    130 rows (two full tiles and one of 2), missing = -999 in the rows, and a matrix of 4 columns (feature 4 is absent).
    -> (image, rows, labels, the restatement's refit, the expected counts from a fresh booster's leaf ids)."""
    js = V.random_booster(8300 + ntree, ntree, 5, max_depth=depth, p_leaf=0.1)
    rng = np.random.default_rng(ntree)
    x = random_rows(rng, 130, 5)
    x[rng.random(x.shape) < 0.1] = SHARED_MISSING
    x = np.ascontiguousarray(x[:, :4])
    y = labels_for(ntree, 130)
    want = R.refit(js, x, SHARED_MISSING, y, 0.5, 1.0, 0)
    trees = V.doc_trees(js)
    fresh = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=SHARED_MISSING)
    counts = V.expected_counts(trees, fresh.predict(d, option_mask=16).reshape(len(x), len(trees)))
    d.free()
    fresh.free()
    V.check_invariants(trees, counts, len(x))
    return js, x, y, want, counts


def count(b, d):
    b.count_visits(d)
    return b.visit_counts()


def refit_is_the_restatement(b, d, y, want, tmp_path, what):
    assert b.refit_leaves(d, y, eta=0.5) == want["leaves_refit"], what
    same_leaves(held(b, tmp_path)[0], (want["value"], want["base_weight"]), what)


def test_counting_and_refitting_in_either_order_share_one_walk(torch_cuda, tmp_path):
    js, x, y, want, counts = shared_walk()
    d = capi.DMatrix(x, missing=SHARED_MISSING)
    b = capi.Booster(model_buffer=js)
    before, seen = count(b, d)                              # the count builds the walk
    assert seen == 130
    V.assert_same_counts(before, counts, "count first")
    refit_is_the_restatement(b, d, y, want, tmp_path, "refit after a count")
    after, seen = b.visit_counts()
    assert seen == 130
    V.assert_same_counts(after, before, "the refit moved a counter")
    b.reset_visit_counts()
    again, seen = count(b, d)                               # the structure is unchanged: so are the counts
    assert seen == 130
    V.assert_same_counts(again, counts, "count after the refit")
    b.free()
    b = capi.Booster(model_buffer=js)
    refit_is_the_restatement(b, d, y, want, tmp_path, "refit first")      # the refit builds the walk
    got, seen = count(b, d)
    assert seen == 130
    V.assert_same_counts(got, counts, "count after a refit that built the walk")
    b.free()
    d.free()


def test_a_visits_knob_between_a_count_and_a_refit(torch_cuda, tmp_path):
    """The plan's tree lists are uploaded again; the walk they index is not."""
    js, x, y, want, counts = shared_walk()
    d = capi.DMatrix(x, missing=SHARED_MISSING)
    b = capi.Booster(model_buffer=js)
    count(b, d)
    b.set_param("ohx_visits_kernel", "lds")
    refit_is_the_restatement(b, d, y, want, tmp_path, "refit after the knob")
    got, seen = count(b, d)
    assert seen == 260
    V.assert_same_counts(got, [c * np.uint64(2) for c in counts], "two counts, the knob between them")
    b.free()
    d.free()


def test_a_model_load_drops_the_shared_walk(torch_cuda, tmp_path):
    js, x, y, want, counts = shared_walk()
    js2, x2, y2, want2, counts2 = shared_walk(5, 3)
    assert len(V.doc_trees(js2)) != len(V.doc_trees(js))
    assert sum(len(v) for v in want2["value"]) != sum(len(v) for v in want["value"])
    d = capi.DMatrix(x, missing=SHARED_MISSING)
    b = capi.Booster(model_buffer=js)
    count(b, d)
    refit_is_the_restatement(b, d, y, want, tmp_path, "the first model")
    d.free()
    b.load_model_buffer(js2)
    d = capi.DMatrix(x2, missing=SHARED_MISSING)
    refit_is_the_restatement(b, d, y2, want2, tmp_path, "the second model")
    got, seen = count(b, d)
    assert seen == 130
    V.assert_same_counts(got, counts2, "the second model")
    b.free()
    d.free()


def test_a_device_move_rebuilds_the_walk_and_both_states(torch_cuda, tmp_path):
    torch = torch_cuda
    if capi.device_count() < 2:
        pytest.skip("one HIP device: nowhere to move the booster")
    js, x, y, want, counts = shared_walk()
    twice = R.refit(R.with_leaves(js, want["value"], want["base_weight"]), x, SHARED_MISSING, y, 0.5, 1.0, 0)
    d = capi.DMatrix(x, missing=SHARED_MISSING)
    b = capi.Booster(model_buffer=js)
    count(b, d)
    refit_is_the_restatement(b, d, y, want, tmp_path, "device 0")
    d.free()
    b.set_param("ohx_device", 1)
    try:
        torch.cuda.set_device(1)                            # a matrix is copied to the current device
        d = capi.DMatrix(x, missing=SHARED_MISSING)
        got, seen = count(b, d)                             # the counters did not move with it
        assert seen == 130
        V.assert_same_counts(got, counts, "device 1")
        refit_is_the_restatement(b, d, y, twice, tmp_path, "device 1")
    finally:
        d.free()
        b.free()
        torch.cuda.set_device(0)


# ---- all or nothing ----

def test_bad_labels_are_refused_with_the_forest_untouched_and_the_next_refit_succeeds(torch_cuda, tmp_path):
    js, _ = adversarial(5)
    n = 1000
    x = rows_for(5, n, -999.0)
    y = labels_for(4, n)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=-999.0)
    margins = b.predict(d, option_mask=1)
    path = str(tmp_path / "before.json")
    b.save_model(path)
    saved = open(path, "rb").read()
    cases = []
    for bad in (float("nan"), 1e30, float("inf")):
        yb = y.copy()
        yb[777] = bad
        cases.append((yb, 1.0, 0.0, "tree 0"))
    # |g| >= 256 at a LATE tree only: every g starts at 120; tree 0 is a root leaf, so with lambda = 0 and eta = 3 its
    # leaf becomes -360 and every g -240; tree 1 is a full tree whose every visited leaf becomes +720: g = 480 at tree 2
    trees = V.doc_trees(js)
    assert len(trees[0]["left_children"]) == 1 and len(trees) > 2
    yl = np.full(n, R.base_of(js) - np.float32(120.0), dtype=np.float32)
    cases.append((yl, 3.0, 0.0, "tree 2"))
    for yb, eta, lam, where in cases:
        with pytest.raises(ValueError, match=where):
            R.refit(js, x, -999.0, yb, eta, lam, 0)
        with pytest.raises(capi.OhxError, match="label") as e:
            b.refit_leaves(d, yb, eta=eta, reg_lambda=lam)
        assert "unchanged" in str(e.value)
        assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(margins))
        b.save_model(path)
        assert open(path, "rb").read() == saved, "a refused refit changed what XGBoosterSaveModel writes"
    want = R.refit(js, x, -999.0, y, 1.0, 1.0, 0)
    assert b.refit_leaves(d, y) == want["leaves_refit"]
    same_leaves(held(b, tmp_path)[0], (want["value"], want["base_weight"]), "after the refusals")
    d.free()
    b.free()


def test_refusals_that_need_a_matrix(torch_cuda, tmp_path):
    js, _ = adversarial(5)
    b = capi.Booster(model_buffer=js)
    (before, _) = held(b, tmp_path)
    d = capi.DMatrix(np.zeros((4, 27), dtype=np.float32), missing=-999.0)
    for nl in (3, 5):
        with pytest.raises(capi.OhxError, match=f"{nl} labels for 4 rows"):
            b.refit_leaves(d, np.zeros(nl, dtype=np.float32))
    wide = capi.DMatrix(np.zeros((4, 28), dtype=np.float32), missing=-999.0)
    with pytest.raises(capi.OhxError, match="Number of columns"):
        b.refit_leaves(wide, np.zeros(4, dtype=np.float32))
    same_leaves(held(b, tmp_path)[0], before, "after the refusals")
    d.free()
    wide.free()


def test_no_rows_too_many_rows_and_an_id_buffer_that_cannot_be_allocated(torch_cuda, tmp_path):
    """Matrices that borrow device memory with a made-up row count: each call is refused before a row or a label is
    read.  2^31 rows are allowed, and 512 trees x 2^31 rows x 4 bytes is 4.4 TB of leaf ids: more than the device has."""
    torch = torch_cuda
    tx = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    ty = torch.zeros(64, dtype=torch.float32, device="cuda")
    y = np.zeros(64, dtype=np.float32)
    js = R.stumps(512)
    b = capi.Booster(model_buffer=js)
    (before, _) = held(b, tmp_path)
    n = C.c_uint64(12345)

    def both_forms(d, nlabel):
        rc = b.lib.OHXBoosterRefitLeaves(b.handle, d.handle, y.ctypes.data, nlabel, 1.0, 1.0, 0, C.byref(n))
        msg = b.lib.XGBGetLastError().decode()
        rc2 = b.lib.OHXBoosterRefitLeavesDevice(b.handle, d.handle, ty.data_ptr(), nlabel, 1.0, 1.0, 0, C.byref(n), None)
        return rc, msg, rc2, b.lib.XGBGetLastError().decode()

    empty = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=0, ncol=3, missing=-999.0)
    rc, msg, rc2, msg2 = both_forms(empty, 0)
    assert rc == rc2 == -1 and "the matrix has no rows" in msg and "the matrix has no rows" in msg2, (msg, msg2)
    many = (1 << 31) + 1
    over = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=many, ncol=3, missing=-999.0)
    rc, msg, rc2, msg2 = both_forms(over, many)
    assert rc == rc2 == -1 and f"at most 2^31 rows per refit ({many} given)" in msg and "at most 2^31 rows" in msg2, (msg, msg2)
    # the device form only: the host form would read 2^31 labels
    most = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=1 << 31, ncol=3, missing=-999.0)
    rc = b.lib.OHXBoosterRefitLeavesDevice(b.handle, most.handle, ty.data_ptr(), 1 << 31, 1.0, 1.0, 0, C.byref(n), None)
    msg = b.lib.XGBGetLastError().decode()
    nbytes = 512 * (1 << 31) * 4
    assert rc == -1 and "leaf-id buffer" in msg and f"512 trees x {1 << 31} rows x 4 = {nbytes} bytes" in msg, msg
    assert n.value == 12345, "a refused call wrote leaves_refit"
    same_leaves(held(b, tmp_path)[0], before, "after the refusals")
    # the booster and its refit state stay usable
    x = np.random.default_rng(3).normal(0, 1, (64, 3)).astype(np.float32)
    want = R.refit(js, x, -999.0, labels_for(1, 64), 1.0, 1.0, 0)
    d = capi.DMatrix(x, missing=-999.0)
    assert b.refit_leaves(d, labels_for(1, 64)) == want["leaves_refit"]
    same_leaves(held(b, tmp_path)[0], (want["value"], want["base_weight"]), "after the refusals, a valid refit")
    for m in (empty, over, most, d):
        m.free()


def test_a_forest_without_trees_has_nothing_to_refit(torch_cuda, tmp_path):
    js = R.stumps(0)
    b = capi.Booster(model_buffer=js)
    x = np.zeros((65, 3), dtype=np.float32)
    d = capi.DMatrix(x, missing=-999.0)
    assert b.refit_leaves(d, np.ones(65, dtype=np.float32)) == 0
    assert np.array_equal(b.predict(d, option_mask=1), np.full(65, R.base_of(js), dtype=np.float32))
    d.free()


# ---- unvisited leaves ----

@pytest.mark.parametrize("unvisited", ["keep", "zero"])
def test_unvisited_leaves_keep_their_value_or_become_zero(torch_cuda, tmp_path, unvisited):
    js, trees = S.contribs_booster(8105, 5)
    x = S.rows_for(17, trees, 64, -999.0)
    y = labels_for(2, 64)
    want = check(tmp_path, js, x, -999.0, y, eta=0.3, unvisited=unvisited, what=unvisited)
    old_v, old_w = R.leaves_of(js)
    rest = seen = 0
    for t, tree in enumerate(V.doc_trees(js)):
        for m in R.leaf_nodes(tree):
            if want["H"][t][m] == 0:
                rest += 1
                if unvisited == "keep":
                    assert helpers.bits(want["value"][t][m]) == helpers.bits(old_v[t][m])
                else:
                    assert helpers.bits(want["value"][t][m]) == 0 and helpers.bits(want["base_weight"][t][m]) == 0, "+0.0f"
            else:
                seen += 1
    assert rest > 0 and seen == want["leaves_refit"], "the batch must leave a leaf unvisited"


# ---- stream capture ----

def test_the_device_form_is_refused_inside_a_capture_and_enqueues_nothing(torch_cuda, tmp_path):
    torch = torch_cuda
    js, _ = adversarial(5)
    x = rows_for(5, 1000, -999.0)
    y = labels_for(4, 1000)
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    b = capi.Booster(model_buffer=js)
    (before, _) = held(b, tmp_path)
    d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=len(x), ncol=27, missing=-999.0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="stream capture"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.refit_leaves_device(d, ty.data_ptr(), len(y), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same_leaves(held(b, tmp_path)[0], before, "the refused call refit")
    want = R.refit(js, x, -999.0, y, 1.0, 1.0, 0)
    with torch.cuda.stream(s):
        n = b.refit_leaves_device(d, ty.data_ptr(), len(y), stream=s.cuda_stream)      # the stream and the booster stay usable
    assert n == want["leaves_refit"]
    same_leaves(held(b, tmp_path)[0], (want["value"], want["base_weight"]), "after the capture")
    d.free()
