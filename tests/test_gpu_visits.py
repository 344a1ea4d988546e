"""Node visit counts on the GPU (csrc/visits.hip) and the covers refreshed from them.  Everything is integer-exact or bit
for bit.

Expected counts never come from the code under test: they are numpy bincount over the leaf ids XGBoosterPredict
(option_mask = 16) returns for the same rows - a path already held to the CPU oracle - summed up each tree by the
tests' own walk (tests/visits_support.py).  On every case a tree's root equals rows_seen and a split the sum of its
children.  Refreshed covers are restated in numpy float32 and checked through what they feed: contributions and
interactions must equal, bit for bit, those of a second booster loaded from the same JSON with sum_hess overwritten by
the test."""
import functools
import json

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import helpers
from tests import visits_support as V
from tests.test_random_forests import random_rows

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 1000, 4097)
# "ohx_visits_kernel": auto counts every tree the global way (the faster of the two at C360, docs/16_visit_counts.md
# 16.4); lds keeps the histogram of every tree that fits in LDS.  A case that does not name a route runs both.
LDS, GLOBAL = ("ohx_visits_kernel", "lds"), ("ohx_visits_kernel", "global")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@functools.lru_cache(maxsize=None)
def adversarial(ntree=10):
    """Every kind of tests/booster_shapes.py (ntree = 10: SMALL_PLANS holds all eight)."""
    js, trees = S.make_booster(7000 + ntree, ntree)
    return js, trees, V.doc_trees(js)


@functools.lru_cache(maxsize=None)
def leaf_beside_long_chain():
    """A root-leaf tree beside a depth-30 chain (contribs_booster's first chain), consistent covers."""
    js, trees = S.contribs_booster(7105, 5)
    depth = max(max(t.depths()) for t in trees)
    assert depth == 30 and any(len(t.left) == 1 for t in trees)
    return js, trees, V.doc_trees(js)


@functools.lru_cache(maxsize=None)
def rows_for(which, n, missing):
    trees = (adversarial() if which == "adversarial" else leaf_beside_long_chain())[1]
    return S.rows_for(n * 3 + 1, trees, n, missing)


def leaf_ids(b, x, missing, ntree):
    d = capi.DMatrix(x, missing=missing)
    ids = b.predict(d, option_mask=16)
    d.free()
    return ids.reshape(len(x), ntree)


def expected(js, x, missing):
    """Counts from the leaf ids of a booster of its own (never one that has counted)."""
    trees = V.doc_trees(js)
    b = capi.Booster(model_buffer=js)
    want = V.expected_counts(trees, leaf_ids(b, x, missing, len(trees)))
    b.free()
    return trees, want


def counted(b, x, missing, params=()):
    for k, v in params:
        b.set_param(k, v)
    d = capi.DMatrix(x, missing=missing)
    b.count_visits(d)
    d.free()
    return b.visit_counts()


def check(js, x, missing, params=None, what=""):
    trees, want = expected(js, x, missing)
    for route in (((), (LDS,)) if params is None else (params,)):
        b = capi.Booster(model_buffer=js)
        got, seen = counted(b, x, missing, route)
        b.free()
        assert seen == len(x), (what, route)
        V.check_invariants(trees, got, len(x))
        V.assert_same_counts(got, want, f"{what} {route}")
    return got


# ---- counts against the existing leaf ids ----

@pytest.mark.parametrize("missing", [-999.0, float("nan")], ids=["missing -999", "missing NaN"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_counts_equal_bincount_of_the_leaf_ids_on_every_kind_of_tree(torch_cuda, n, missing):
    """All KINDS, tie rows, NaN and -999 in the rows (rows_for: random_rows + tie rows)."""
    js, trees, _ = adversarial()
    assert {k for k in S.SMALL_PLANS[10]} == set(S.KINDS)
    x = rows_for("adversarial", n, missing)
    if n >= 1000:
        assert np.isnan(x).any() and (x == -999.0).any()
    check(js, x, missing, what=f"{n} rows")


def test_the_golden_hand_forest_against_its_recorded_leaf_ids(torch_cuda):
    """tests/golden: five hand-made trees (three of them root leaves) and the leaf ids recorded for the hand cases."""
    import os
    js = open(os.path.join(helpers.GOLDEN, "hand_forest.json"), "rb").read()
    cases, x = helpers.load_hand_cases()
    trees = V.doc_trees(js)
    want = V.expected_counts(trees, np.asarray(cases["leaf_index"], dtype=np.float32))
    for params in ((), (GLOBAL,), (LDS,), (LDS, ("ohx_visits_lds_leaves", 1))):
        b = capi.Booster(model_buffer=js)
        got, seen = counted(b, x, cases["missing"], params)
        assert seen == len(x)
        V.check_invariants(trees, got, len(x))
        V.assert_same_counts(got, want, str(params))
        b.free()


@pytest.mark.parametrize("n", (65, 1000))
def test_a_root_leaf_beside_a_depth_30_chain(torch_cuda, n):
    js, _, _ = leaf_beside_long_chain()
    check(js, rows_for("chain", n, -999.0), -999.0)


@pytest.mark.parametrize("ncol", (1, 20, 26))
def test_fewer_columns_than_features(torch_cuda, ncol):
    """The columns the matrix lacks are missing: the default child everywhere they are split on."""
    js, _, _ = adversarial()
    x = np.ascontiguousarray(rows_for("adversarial", 1000, -999.0)[:, :ncol])
    check(js, x, -999.0, what=f"{ncol} columns")


@pytest.mark.parametrize("nfeat,staged", [(100, True), (300, False)], ids=["100 features", "tiles that do not fit LDS"])
def test_other_feature_counts(torch_cuda, nfeat, staged):
    js = V.random_booster(7200 + nfeat, 4, nfeat, max_depth=8, p_leaf=0.15)
    assert synth.visits_plan(js)["stage"] == staged
    rng = np.random.default_rng(nfeat)
    x = random_rows(rng, 1000, nfeat)
    x[rng.random(x.shape) < 0.02] = -999.0
    for params in ((), (LDS,), (LDS, ("ohx_visits_lds_leaves", 8))):
        check(js, x, -999.0, params, what=f"{nfeat} features {params}")
    check(js, np.ascontiguousarray(x[:, :nfeat - 3]), -999.0, what="three columns short")


def test_more_columns_than_features_are_refused(torch_cuda):
    js, _, _ = adversarial()
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(np.zeros((4, 28), dtype=np.float32), missing=-999.0)
    with pytest.raises(capi.OhxError, match="Number of columns"):
        b.count_visits(d)
    assert b.visit_counts()[1] == 0


# ---- past the launch caps ----

def test_more_rows_than_two_trips_of_each_kernels_loop(torch_cuda):
    """A block strides over the tiles.  One trip of the LDS kernel's loop takes CUs x 1 block x 256 rows per tree, of the
    global kernel's CUs x 4 blocks x 256 rows: more than twice the larger, through both kernels."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    trip_lds = cus * capi.VISITS_LDS_BLOCKS_PER_CU * capi.VISITS_BLOCK_ROWS
    trip_global = cus * capi.VISITS_GLOBAL_BLOCKS_PER_CU * capi.VISITS_BLOCK_ROWS
    n = 2 * max(trip_lds, trip_global) + 77
    assert n > 2 * trip_lds and n > 2 * trip_global and n % 64 != 0
    js, _ = S.make_booster(7303, 3)
    trees = V.doc_trees(js)
    assert len(trees) == 3
    p = synth.visits_plan(js, num_cus=cus, ntiles=(n + 63) // 64)
    assert (n + 63) // 64 > 2 * 4 * p["lds_blocks"] and (n + 63) // 64 > 2 * 4 * p["global_blocks"]
    rng = np.random.default_rng(5)
    x = rng.normal(0, 2, (n, 27)).astype(np.float32)
    x[rng.random(x.shape) < 0.01] = np.nan
    _, want = expected(js, x, float("nan"))
    for params in ((LDS,), (GLOBAL,)):
        b = capi.Booster(model_buffer=js)
        got, seen = counted(b, x, float("nan"), params)
        b.free()
        assert seen == n
        V.check_invariants(trees, got, n)
        V.assert_same_counts(got, want, str(params))


# ---- the same integers whatever the route ----

def test_the_lds_and_the_global_way_and_every_capacity_agree(torch_cuda):
    js, _, trees = adversarial()
    x = rows_for("adversarial", 4097, -999.0)
    leaves = [sum(1 for m in V.reachable(t) if t["left_children"][m] == -1) for t in trees]
    assert min(leaves) == 1 and any(1 < v <= 8 for v in leaves) and max(leaves) > 8, "1 and 8 mix both ways"
    first = None
    for params in ((), (GLOBAL,), (("ohx_visits_kernel", "auto"),), (LDS,), (LDS, ("ohx_visits_lds_leaves", 1)),
                   (LDS, ("ohx_visits_lds_leaves", 8)), (LDS, ("ohx_visits_lds_leaves", "auto"))):
        got = check(js, x, -999.0, params, what=str(params))
        first = first or got
        V.assert_same_counts(got, first, str(params))


def test_a_knob_changed_between_two_counts_keeps_adding_to_the_same_counters(torch_cuda):
    js, _, trees = adversarial()
    x = rows_for("adversarial", 1000, -999.0)
    _, want = expected(js, x, -999.0)
    b = capi.Booster(model_buffer=js)
    counted(b, x, -999.0, (LDS,))
    counted(b, x, -999.0, (("ohx_visits_lds_leaves", 8),))
    got, seen = counted(b, x, -999.0, (GLOBAL,))
    assert seen == 3000
    V.check_invariants(trees, got, 3000)
    V.assert_same_counts(got, [w * np.uint64(3) for w in want])


@pytest.mark.parametrize("grid", [(12, 10, 0, 1200), (12, 10, 2 * 120 + 37, 1000), (7, 5, 35 * 3 + 4, 333), (64, 1, 0, 640)],
                         ids=["whole levels", "a shard that starts inside a level", "odd extents", "level size only"])
def test_with_and_without_the_grid_said(torch_cuda, grid):
    im, jm, row0, n = grid
    js, _, trees = adversarial()
    x = rows_for("adversarial", 4097, -999.0)[:n]
    _, want = expected(js, x, -999.0)
    for params in ((), (LDS,), (LDS, ("ohx_brick", "8,4,2")), (("ohx_brick_k_fastest", 0),)):
        for said in (False, True):
            b = capi.Booster(model_buffer=js)
            for k, v in params:
                b.set_param(k, v)
            d = capi.DMatrix(x, missing=-999.0)
            if said:
                d.set_grid(im, jm, row0)
            b.count_visits(d)
            got, seen = b.visit_counts()
            d.free()
            b.free()
            assert seen == n
            V.check_invariants(trees, got, n)
            V.assert_same_counts(got, want, f"{params} grid said: {said}")


def test_host_form_and_device_form_on_a_stream_of_the_callers(torch_cuda):
    torch = torch_cuda
    js, _, trees = adversarial()
    x = rows_for("adversarial", 4097, float("nan"))
    _, want = expected(js, x, float("nan"))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(x).to("cuda", non_blocking=False)
    s.synchronize()
    b = capi.Booster(model_buffer=js)
    b.set_param(*LDS)
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=len(x), ncol=27, missing=float("nan"))
    b.count_visits_device(d, stream=s.cuda_stream)
    got, seen = b.visit_counts(stream=s.cuda_stream)          # waits for the stream
    assert seen == len(x)
    V.check_invariants(trees, got, len(x))
    V.assert_same_counts(got, want, "device form")
    # the host form on the same borrowed rows adds the same again
    b.count_visits(d)
    got, seen = b.visit_counts()
    assert seen == 2 * len(x)
    V.assert_same_counts(got, [w * np.uint64(2) for w in want], "host form on a device matrix")
    d.free()
    b.free()


# ---- accumulation ----

def test_two_halves_equal_the_whole_reset_gives_zeros_and_a_model_load_drops_the_counts(torch_cuda):
    js, _, trees = adversarial()
    x = rows_for("adversarial", 4097, -999.0)
    _, want = expected(js, x, -999.0)
    b = capi.Booster(model_buffer=js)
    got, seen = counted(b, x[:2000], -999.0, (LDS,))
    assert seen == 2000
    V.check_invariants(trees, got, 2000)
    got, seen = counted(b, x[2000:], -999.0, (GLOBAL,))
    assert seen == 4097
    V.assert_same_counts(got, want, "two halves")
    b.reset_visit_counts()
    got, seen = b.visit_counts()
    assert seen == 0 and all(not c.any() for c in got)
    got, seen = counted(b, x, -999.0)
    assert seen == 4097
    V.assert_same_counts(got, want, "after a reset")
    b.load_model_buffer(js)
    got, seen = b.visit_counts()
    assert seen == 0 and all(not c.any() for c in got)
    with pytest.raises(capi.OhxError, match="no row has been counted yet"):
        b.refresh_cover(0.0)
    got, seen = counted(b, x[:65], -999.0)
    assert seen == 65
    V.assert_same_counts(got, expected(js, x[:65], -999.0)[1], "after a model load")
    b.free()


def test_release_scratch_leaves_the_counts_alone(torch_cuda):
    js, _, _ = adversarial()
    x = rows_for("adversarial", 1000, -999.0)
    b = capi.Booster(model_buffer=js)
    got, _ = counted(b, x, -999.0)
    assert b.lib.OHXReleaseScratch() == 0
    again, seen = b.visit_counts()
    assert seen == 1000
    V.assert_same_counts(again, got)
    b.free()


# ---- refresh ----

@functools.lru_cache(maxsize=None)
def small_forest():
    """Full shallow trees of 8 features, no feature twice on a path: a batch of 3000 rows passes every split (asserted
    where it is used, from the leaf ids)."""
    return V.level_forest(7400, 6, 8, depth=3)


def explain_all(b, x, missing):
    d = capi.DMatrix(x, missing=missing)
    out = [b.predict_contribs(d), b.predict_contribs(d, approximate=True), b.predict_interactions(d),
           b.predict_interactions(d, approximate=True)]
    d.free()
    return out


REFRESH_CASES = [("small", 0.0), ("small", 0.5), ("long chain", 0.5)]


@pytest.mark.parametrize("which,prior_weight", REFRESH_CASES, ids=[f"{w} {p}" for w, p in REFRESH_CASES])
def test_refreshed_covers_feed_contributions_and_interactions_bit_for_bit(torch_cuda, tmp_path, which, prior_weight):
    if which == "small":
        js, missing = small_forest(), -999.0
        rng = np.random.default_rng(9)
        x = random_rows(rng, 3000, 8)
    else:
        js, missing = leaf_beside_long_chain()[0], -999.0
        x = rows_for("chain", 1000, missing)
    trees, want = expected(js, x, missing)
    if prior_weight == 0.0:
        assert not V.zero_count_splits(trees, want), "the batch must pass every split for prior_weight = 0"
    covers = [V.expected_cover(t, c, prior_weight) for t, c in zip(trees, want)]
    xe = x[:96]                                        # the rows that are explained
    b = capi.Booster(model_buffer=js)
    dm = capi.DMatrix(x, missing=missing)
    margin_before = b.predict(dm, option_mask=1)
    before = explain_all(b, xe, missing)               # the contributions state exists and holds the OLD covers
    b.count_visits(dm)
    b.refresh_cover(prior_weight)
    margin_after = b.predict(dm, option_mask=1)
    assert np.array_equal(helpers.bits(margin_before), helpers.bits(margin_after))
    assert np.array_equal(leaf_ids(b, x, missing, len(trees)), leaf_ids(capi.Booster(model_buffer=js), x, missing, len(trees)))
    got = explain_all(b, xe, missing)
    other = capi.Booster(model_buffer=V.with_covers(js, covers))
    ref = explain_all(other, xe, missing)
    for g, r, o, name in zip(got, ref, before, ("exact", "approximate", "interactions", "approximate interactions")):
        assert g.shape == r.shape and np.array_equal(helpers.bits(g), helpers.bits(r)), name
    assert any(not np.array_equal(helpers.bits(g), helpers.bits(o)) for g, o in zip(got, before)), "the covers changed nothing"
    # the counters are kept
    kept, seen = b.visit_counts()
    assert seen == len(x)
    V.assert_same_counts(kept, want, "after the refresh")
    # the new covers are held by all three file formats
    flat = np.concatenate(covers)
    for ext in ("json", "ubj", "bin"):
        path = str(tmp_path / f"refreshed.{ext}")
        b.save_model(path)
        again = capi.Booster(model_file=path)
        back = str(tmp_path / f"back_{ext}.json")
        again.save_model(back)
        held = np.concatenate([np.asarray(t["sum_hessian"], dtype=np.float32) for t in V.doc_trees(open(back, "rb").read())])
        assert np.array_equal(helpers.bits(held), helpers.bits(flat)), ext
        again.free()
    dm.free()


def test_a_second_refresh_blends_the_refreshed_covers(torch_cuda):
    js = small_forest()
    x = random_rows(np.random.default_rng(9), 3000, 8)
    trees, want = expected(js, x, -999.0)
    b = capi.Booster(model_buffer=js)
    counted(b, x, -999.0)
    b.refresh_cover(0.5)
    b.refresh_cover(0.25)
    once = [V.expected_cover(t, c, 0.5) for t, c in zip(trees, want)]
    mid = V.doc_trees(V.with_covers(js, once))
    twice = [V.expected_cover(t, c, 0.25) for t, c in zip(mid, want)]
    other = capi.Booster(model_buffer=V.with_covers(js, twice))
    for g, r in zip(explain_all(b, x[:64], -999.0), explain_all(other, x[:64], -999.0)):
        assert np.array_equal(helpers.bits(g), helpers.bits(r))


def test_zero_count_splits_refuse_a_plain_refresh_and_pass_with_a_prior(torch_cuda):
    js, _, trees = leaf_beside_long_chain()
    x = rows_for("chain", 64, -999.0)
    _, want = expected(js, x, -999.0)
    zero = V.zero_count_splits(trees, want)
    assert zero, "the batch must leave a split unvisited"
    nsplit = sum(1 for t in trees for m in V.reachable(t) if t["left_children"][m] != -1)
    original = explain_all(capi.Booster(model_buffer=js), x, -999.0)
    b = capi.Booster(model_buffer=js)
    counted(b, x, -999.0)
    with pytest.raises(capi.OhxError) as e:
        b.refresh_cover(0.0)
    msg = str(e.value)
    assert f"node {zero[0][1]} of tree {zero[0][0]}" in msg and f"{len(zero)} of {nsplit} splits" in msg and "prior_weight" in msg, msg
    for g, r in zip(explain_all(b, x, -999.0), original):
        assert np.array_equal(helpers.bits(g), helpers.bits(r)), "a refused refresh changed the forest"
    b.refresh_cover(1e-3)
    after = explain_all(b, x, -999.0)
    for g in after:
        assert np.all(np.isfinite(g))
    covers = [V.expected_cover(t, c, 1e-3) for t, c in zip(trees, want)]
    for g, r in zip(after, explain_all(capi.Booster(model_buffer=V.with_covers(js, covers)), x, -999.0)):
        assert np.array_equal(helpers.bits(g), helpers.bits(r))


# ---- stream capture and graphs captured earlier ----

def test_the_device_form_is_refused_inside_a_capture_and_enqueues_nothing(torch_cuda):
    torch = torch_cuda
    js, _, trees = adversarial()
    x = rows_for("adversarial", 1000, -999.0)
    _, want = expected(js, x, -999.0)
    t = torch.from_numpy(x).cuda()
    b = capi.Booster(model_buffer=js)
    b.set_param(*LDS)
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=len(x), ncol=27, missing=-999.0)
    b.count_visits_device(d)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="stream capture"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.count_visits_device(d, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, seen = b.visit_counts()
    assert seen == len(x)
    V.assert_same_counts(got, want, "the refused call counted")
    with torch.cuda.stream(s):
        b.count_visits_device(d, stream=s.cuda_stream)          # the stream and the booster stay usable
    got, seen = b.visit_counts(stream=s.cuda_stream)
    assert seen == 2 * len(x)
    V.assert_same_counts(got, [w * np.uint64(2) for w in want])
    d.free()


def test_a_graph_captured_earlier_still_replays_after_a_count(torch_cuda, small_model):
    """The visit state has buffers of its own: a captured predict holds raw pointers to the booster's."""
    torch = torch_cuda
    grid = (12, 72, 72)
    nrow = 12 * 72 * 40
    x = synth.rows_cpu(grid, 0, nrow)
    x[::97, 5] = synth.XX_MISS
    want_margin = helpers.oracle_predict(small_model.image, x, synth.XX_MISS)
    rows = torch.from_numpy(x).cuda()
    out = torch.zeros(nrow, dtype=torch.float32, device="cuda")
    b = capi.Booster(model_buffer=small_model.image)
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=nrow, ncol=27, missing=synth.XX_MISS)
    d.set_grid(grid[0], grid[1], 0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.predict_device(d, out.data_ptr(), stream=s.cuda_stream)          # the plain call that makes the buffers
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.predict_device(d, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    assert np.array_equal(helpers.bits(first), helpers.bits(want_margin))
    ntree = b.info()["num_trees"]
    ids = torch.zeros(nrow * ntree, dtype=torch.float32, device="cuda")
    b.predict_device(d, ids.data_ptr(), option_mask=16)
    torch.cuda.synchronize()
    b.set_param(*LDS)
    b.count_visits_device(d, stream=s.cuda_stream)
    b.set_param(*GLOBAL)
    b.count_visits(d)
    got, seen = b.visit_counts(stream=s.cuda_stream)
    js = bytes(synth.convert_model(small_model.image, "json"))
    trees = V.doc_trees(js)
    V.check_invariants(trees, got, 2 * nrow)
    want = V.expected_counts(trees, ids.cpu().numpy().reshape(nrow, ntree))
    V.assert_same_counts(got, [w * np.uint64(2) for w in want], "the OH-shaped booster on bricks")
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    b.check()
    assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(first))
    d.free()
