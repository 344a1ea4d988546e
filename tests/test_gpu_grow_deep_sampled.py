"""Row and column subsampling for trees deeper than eight levels on the GPU (csrc/grow_deep.hip,
OHXBoosterBoostTreesDeepSampled).  Every array of every new tree, nodes_added, rounds_run and best_round are compared as
integers or bit for bit, both RMSE arrays with ==, and models byte for byte.

The expected values are the restatement's (tests/grow_deep_sampled_support.py: grow_sampled_support.boost_sampled, whose
level loop has no cap) and, where the header states an equality, another call on a twin booster: the Deep call at
(1, 1), the Sampled call up to depth 8, and the Deep call given the bag as 0 / 1 weights and the cuts of the unselected
features emptied.  The model of every case has no tree, so the margin a restatement starts from is the model's base.
What a case is meant to reach - a level beyond 7, more open nodes than a batch holds, a list shorter than the features,
a bag strictly inside the rows - is asserted from the restatement before the GPU is asked."""
import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_deep_sampled_support as DS
from tests import grow_deep_support as D
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests import helpers
from tests.test_gpu_grow import held, same_new_trees
from tests.test_gpu_grow_eval import same_result, saved

pytestmark = pytest.mark.gpu

NAN = float("nan")
BLOCK = 256          # lanes of split phase 1's block (csrc/grow.hpp kGrowBlock)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def model(nfeat=3):
    return G.empty_model(nfeat, base=DS.BASE)


def restate(x, missing, y, w, cuts, nfeat, ev=None, pred=None, tree0=0, **kw):
    """ev: (rows, missing, labels, weights or None).  Keyword names as the Python binding's."""
    pk = {"rounds": kw.get("rounds", 1), "max_depth": kw.get("max_depth", 12), "eta": kw.get("eta", 0.3),
          "lam": kw.get("reg_lambda", 1.0), "gamma": kw.get("gamma", 0.0),
          "min_child_weight": kw.get("min_child_weight", 1.0), "patience": kw.get("patience", 0),
          "subsample": kw.get("subsample", 1.0), "colsample_bytree": kw.get("colsample_bytree", 1.0), "seed": kw.get("seed", 0)}
    ep = np.full(len(ev[2]), DS.BASE, np.float32) if ev is not None else None
    start = np.full(len(y), DS.BASE, np.float32) if pred is None else pred
    return DS.boost_deep_sampled(start, x, missing, y, w, cuts, nfeat, eval_set=ev, eval_pred=ep, tree0=tree0, **pk)


def run(tmp_path, want, x, missing, y, w, cuts, nfeat, ev=None, what="", **kw):
    """One host-form call on a fresh booster against the restated `want` -> (the result, the booster, the matrices)."""
    b = capi.Booster(model_buffer=model(nfeat))
    d = capi.DMatrix(x, missing=missing)
    ed = capi.DMatrix(ev[0], missing=ev[1]) if ev is not None else None
    got = b.boost_trees_deep_sampled(d, y, cuts, weights=w, eval_set=(ed, ev[2], ev[3]) if ev is not None else None, **kw)
    same_result(got, want, what)
    same_new_trees(held(b, tmp_path)[0], want["trees"], 0, what)
    return got, b, [m for m in (d, ed) if m is not None]


def done(b, mats):
    for m in mats:
        m.free()
    b.free()


def deep_levels(t):
    """(open nodes, splits) of the levels from 8 on."""
    return D.levels(t)[8:]


# ---- against the restatement ----

def test_several_batches_and_chunks_over_half_the_rows_and_three_of_five_features(torch_cuda, tmp_path):
    x, y, w, cuts, ev, want = DS.restated(40000, 40014, 14, 64, 0.0, 0.0, 0.5, 0.7, 5, rounds=2, nfeat=5)
    batch = synth.grow_deep_batch()
    for t, bag, feats in zip(want["trees"], want["bags"], want["features"]):
        lv = D.levels(t)
        assert len(feats) == 3 and 0 < bag.sum() < 40000 and D.depth_of(t) == 14
        assert sum(o > batch for o, _ in lv) >= 2 and max(o for o, _ in lv) > BLOCK, "several batches, several chunks"
        assert set(t["feature"][t["left"] >= 0].tolist()) <= set(feats)
    assert not np.array_equal(want["bags"][0], want["bags"][1]), "a second bag is drawn"
    assert want["features"][0] != want["features"][1], "and a second list"
    kw = dict(rounds=2, max_depth=14, eta=0.5, reg_lambda=0.0, min_child_weight=0.0, subsample=0.5, colsample_bytree=0.7, seed=5)
    got, b, mats = run(tmp_path, want, x, NAN, y, None, cuts, 5, what="several batches", **kw)
    assert got["nodes_added"] == sum(len(t["left"]) for t in want["trees"]) > 10000
    done(b, mats)


def test_depth_18_with_a_held_out_set_weights_and_patience(torch_cuda, tmp_path):
    x, y, w, cuts, ev, want = DS.restated(12000, 12018, 18, 16, 0.0, 0.0, 0.5, 1.0, 3, rounds=4, weighted=True, held_out=3000,
                                          patience=2)
    assert set(np.unique(w)) == {0.0, 0.5, 1.0, 1.5, 2.0} and set(np.unique(ev[3])) == {0.0, 0.5, 1.0, 1.5, 2.0}
    first = want["all_trees"][0]
    assert D.depth_of(first) == 18 and all(s > 0 for _, s in D.levels(first)[:18]), "splits at every level 0..17"
    assert np.count_nonzero(want["bags"][0] & (w == 0.0)) > 500, "zero-weight rows in the bag"
    assert want["features"][0] == [0, 1, 2] and 0 < want["bags"][0].sum() < 12000
    kw = dict(rounds=4, max_depth=18, eta=0.5, reg_lambda=0.0, min_child_weight=0.0, patience=2, subsample=0.5, seed=3)
    got, b, mats = run(tmp_path, want, x, NAN, y, w, cuts, 3, ev=ev, what="depth 18, held-out, weights", **kw)
    assert len(got["eval_rmse"]) == want["rounds_run"] + 1
    # the held-out margin of the kept trees, by the predict path
    assert np.array_equal(helpers.bits(b.predict(mats[1], option_mask=1)), helpers.bits(want["eval_pred"]))
    done(b, mats)


@pytest.mark.parametrize("subsample,colsample", [(1.0, 0.67), (0.5, 1.0)])
def test_one_fraction_alone(torch_cuda, tmp_path, subsample, colsample):
    """A NULL bag with a list, and a bag with the full list."""
    x, y, w, cuts, ev, want = DS.restated(4097, 4097, 12, 255, 1.0, 0.0, subsample, colsample, 9, rounds=2)
    for t, bag, feats in zip(want["trees"], want["bags"], want["features"]):
        assert (subsample == 1.0) == bool(bag.all()) and len(feats) == (2 if colsample < 1 else 3)
        assert D.depth_of(t) > 8 and deep_levels(t)[0][1] > 0, "level 8 splits"
    kw = dict(rounds=2, max_depth=12, eta=0.5, reg_lambda=1.0, min_child_weight=0.0, subsample=subsample,
              colsample_bytree=colsample, seed=9)
    got, b, mats = run(tmp_path, want, x, NAN, y, None, cuts, 3, what=f"({subsample}, {colsample})", **kw)
    done(b, mats)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097 + 65536 + 1))
def test_row_counts_at_depth_18(torch_cuda, tmp_path, n):
    """The rows run out and the tree ends through the level word; a last bag word that is not full; a row count that
    is no multiple of 64."""
    rounds = 2 if n < 100 else 1
    x, y, cuts = D.inputs(n, 100 + n, bins=255 if n < 100 else 32)
    w = np.random.default_rng(n).choice(np.asarray((0.5, 1.0, 2.0), np.float32), n)
    # one row: a seed whose bags hold it (the empty bag is among the refusals)
    seed = next(s for s in range(n, n + 64) if n > 1 or all(P.bag(s, i, 1, 0.5)[0] for i in range(rounds)))
    kw = dict(rounds=rounds, max_depth=18, eta=0.5, reg_lambda=0.0, min_child_weight=0.0, subsample=0.5, seed=seed)
    want = restate(x, NAN, y, w, cuts, 3, **kw)
    for t, bag in zip(want["trees"], want["bags"]):
        assert len(t["left"]) <= 2 * int(bag.sum()) - 1, "every leaf holds a row of the bag"
        if n < 100:
            assert D.depth_of(t) < 18, "the rows run out before the depth does"
        else:
            assert D.depth_of(t) > 12 and max(o for o, _ in deep_levels(t)) > synth.grow_deep_batch() and n % 64 == 2
    if n >= 63:
        assert all(0 < m.sum() < n for m in want["bags"])
    got, b, mats = run(tmp_path, want, x, NAN, y, w, cuts, 3, what=f"{n} rows", **kw)
    done(b, mats)


@pytest.mark.parametrize("nfeat,bins,colsample,n_sel", [(27, 64, 0.5, 13), (128, 8, 0.3, 38), (128, 8, 1.0 / 128.0, 1)])
def test_feature_counts_and_the_packing_at_depth_10(torch_cuda, tmp_path, nfeat, bins, colsample, n_sel):
    """13 of 27; 38 of 128: a second group of columns whose last packed word is not full; and one feature of 128."""
    x, y, cuts = D.inputs(4097, 7 + nfeat, nfeat=nfeat, bins=bins)
    kw = dict(rounds=2, max_depth=10, eta=0.5, reg_lambda=1.0, min_child_weight=2.0, subsample=0.8, colsample_bytree=colsample, seed=21)
    want = restate(x, NAN, y, None, cuts, nfeat, **kw)
    assert all(len(f) == n_sel for f in want["features"]) and want["features"][0] != want["features"][1]
    assert n_sel % 4 != 0 and n_sel % 32 != 0
    for t, feats in zip(want["trees"], want["features"]):
        assert set(t["feature"][t["left"] >= 0].tolist()) <= set(feats)
        if n_sel > 1:
            assert D.depth_of(t) == 10
        else:
            assert 0 < D.depth_of(t) < 8, "seven cuts of one feature: the tree ends before the deep levels, through the level word"
        if n_sel > 32:
            assert max(t["feature"][t["left"] >= 0].tolist()) >= feats[32], "a feature of the second group of columns wins a split"
    got, b, mats = run(tmp_path, want, x, NAN, y, None, cuts, nfeat, what=f"{n_sel} of {nfeat} features", **kw)
    done(b, mats)


def test_minus_999_missing_and_fewer_columns_than_features(torch_cuda, tmp_path):
    x, y, _ = D.inputs(4097, 31, nfeat=3, bins=64, missing=-999.0)
    assert np.count_nonzero(x == -999.0) > 300 and not np.isnan(x).any()
    cuts3 = G.quantile_cuts(x, -999.0, 64)
    # a booster of 5 features over rows of 3 columns: features 3 and 4 are missing everywhere and have no cut
    cuts = (np.concatenate([cuts3[0], [cuts3[0][-1]] * 2]).astype(np.uint64), cuts3[1])
    kw = dict(rounds=3, max_depth=11, eta=0.5, reg_lambda=1.0, min_child_weight=0.0, subsample=0.6, colsample_bytree=0.6, seed=2)
    want = restate(x, -999.0, y, None, cuts, 5, **kw)
    assert all(len(f) == 3 for f in want["features"])
    assert any(set(f) & {3, 4} for f in want["features"]), "a list that holds a feature without a column"
    assert max(D.depth_of(t) for t in want["trees"]) == 11 and all(t["feature"].max() <= 2 for t in want["trees"])
    got, b, mats = run(tmp_path, want, x, -999.0, y, None, cuts, 5, what="-999, 3 of 5 columns", **kw)
    done(b, mats)


# ---- the header's equalities, against other calls on a twin booster ----

@pytest.mark.parametrize("seed", (0, 7))
def test_all_rows_and_all_features_leave_what_the_deep_call_leaves(torch_cuda, tmp_path, seed):
    x, y, w, cuts, ev, _ = D.restated(4097, 4097, 12, 255, 1.0, 0.0, rounds=2, weighted=True, held_out=1300)
    ex, _, ey, ew = ev
    d, ed = capi.DMatrix(x, missing=NAN), capi.DMatrix(ex, missing=NAN)
    kw = dict(rounds=2, max_depth=12, eta=0.5, reg_lambda=1.0, min_child_weight=0.0)
    twin, b = capi.Booster(model_buffer=model()), capi.Booster(model_buffer=model())
    want = twin.boost_trees_deep(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **kw)
    got = b.boost_trees_deep_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, ew), subsample=1.0, colsample_bytree=1.0, seed=seed, **kw)
    assert saved(b, tmp_path) == saved(twin, tmp_path), "bytes in three formats"
    for k in ("train_rmse", "eval_rmse"):
        assert got[k].tolist() == want[k].tolist(), k
    assert (got["nodes_added"], got["rounds_run"], got["best_round"]) == (want["nodes_added"], want["rounds_run"], want["best_round"])
    assert got["nodes_added"] > 2 * 511, "both trees go past level 8"
    done(twin, [])
    done(b, [d, ed])


@pytest.mark.parametrize("max_depth", (3, 8))
def test_up_to_depth_8_the_call_leaves_what_the_sampled_call_leaves(torch_cuda, tmp_path, max_depth):
    x, y, cuts = D.inputs(4097, 55, bins=64)
    ex, ey, _ = D.inputs(700, 56, bins=64)
    rng = np.random.default_rng(3)
    w, ew = (rng.random(4097) * 3).astype(np.float32), (rng.random(700) * 3).astype(np.float32)
    d, ed = capi.DMatrix(x, missing=NAN), capi.DMatrix(ex, missing=NAN)
    kw = dict(rounds=3, max_depth=max_depth, eta=0.5, reg_lambda=1.0, patience=2, min_child_weight=0.5, subsample=0.5,
              colsample_bytree=0.7, seed=13)
    twin, b = capi.Booster(model_buffer=model()), capi.Booster(model_buffer=model())
    want = twin.boost_trees_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **kw)
    got = b.boost_trees_deep_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **kw)
    assert saved(b, tmp_path) == saved(twin, tmp_path)
    for k in ("train_rmse", "eval_rmse"):
        assert got[k].tolist() == want[k].tolist(), k
    assert (got["nodes_added"], got["rounds_run"], got["best_round"]) == (want["nodes_added"], want["rounds_run"], want["best_round"])
    assert got["nodes_added"] > 3 * max_depth
    done(twin, [])
    done(b, [d, ed])


@pytest.mark.parametrize("subsample,colsample", [(0.5, 0.7), (1.0, 0.4)])
def test_one_round_is_the_deep_call_with_the_bag_as_weights_and_emptied_cuts(torch_cuda, tmp_path, subsample, colsample):
    x, y, cuts = D.inputs(4097, 77, nfeat=5, bins=64)
    w = np.random.default_rng(8).choice(np.asarray((0.0, 0.5, 1.0, 2.0), np.float32), 4097)
    seed = 11
    mask, kept = P.bag(seed, 0, 4097, subsample), P.features(seed, 0, 5, colsample)
    assert (subsample == 1.0) == bool(mask.all()) and len(kept) == P.num_selected(5, colsample) < 5
    kw = dict(rounds=1, max_depth=13, eta=0.5, reg_lambda=1.0, min_child_weight=0.0)
    stated = restate(x, NAN, y, w, cuts, 5, subsample=subsample, colsample_bytree=colsample, seed=seed, **kw)
    assert D.depth_of(stated["trees"][0]) > 8 and deep_levels(stated["trees"][0])[0][1] > 0, "level 8 splits"
    d = capi.DMatrix(x, missing=NAN)
    twin, b = capi.Booster(model_buffer=model(5)), capi.Booster(model_buffer=model(5))
    want = twin.boost_trees_deep(d, y, P.emptied_cuts(cuts, 5, kept), weights=(w * mask).astype(np.float32), **kw)
    got = b.boost_trees_deep_sampled(d, y, cuts, weights=w, subsample=subsample, colsample_bytree=colsample, seed=seed, **kw)
    assert got["nodes_added"] == want["nodes_added"] == stated["nodes_added"]
    assert saved(b, tmp_path) == saved(twin, tmp_path)
    done(twin, [])
    done(b, [d])


# ---- the draw, and what changes nothing ----

def test_a_longer_forest_moves_the_draw(torch_cuda, tmp_path):
    """A second call on one booster starts at T0 = 2: its bags and lists are those of trees 2 and 3."""
    x, y, w, cuts, ev, want = DS.restated(4097, 4097, 12, 255, 1.0, 0.0, 0.5, 0.67, 9, rounds=2)
    kw = dict(rounds=2, max_depth=12, eta=0.5, reg_lambda=1.0, min_child_weight=0.0, subsample=0.5, colsample_bytree=0.67, seed=9)
    got, b, (d,) = run(tmp_path, want, x, NAN, y, None, cuts, 3, what="first call", **kw)
    more = restate(x, NAN, y, None, cuts, 3, pred=want["pred"], tree0=2, **kw)
    assert not np.array_equal(more["bags"][0], want["bags"][0]) and np.array_equal(more["bags"][0], P.bag(9, 2, 4097, 0.5))
    path = str(tmp_path / "two_trees.json")
    b.save_model(path)
    again = b.boost_trees_deep_sampled(d, y, cuts, **kw)
    same_result(again, more, "second call")
    same_new_trees(held(b, tmp_path)[0], want["trees"] + more["trees"], 0, "second call")
    # a first call on a booster loaded with those two trees: the same draw, from the margin of a predict
    loaded = capi.Booster(model_file=path)
    same_result(loaded.boost_trees_deep_sampled(d, y, cuts, **kw), more, "a forest as loaded")
    assert saved(loaded, tmp_path) == saved(b, tmp_path)
    loaded.free()
    done(b, [d])


def test_permuted_rows_are_the_restatement_of_the_permuted_matrix(torch_cuda, tmp_path):
    x, y, w, cuts, ev, want = DS.restated(4097, 4097, 12, 255, 1.0, 0.0, 0.5, 0.67, 9, rounds=2)
    perm = np.random.default_rng(1).permutation(4097)
    xp, yp = np.ascontiguousarray(x[perm]), y[perm].copy()
    kw = dict(rounds=2, max_depth=12, eta=0.5, reg_lambda=1.0, min_child_weight=0.0, subsample=0.5, colsample_bytree=0.67, seed=9)
    wantp = restate(xp, NAN, yp, None, cuts, 3, **kw)
    assert wantp["train_rmse"] != want["train_rmse"], "other rows are drawn: r is the row's place in the matrix"
    got, b, mats = run(tmp_path, wantp, xp, NAN, yp, None, cuts, 3, what="rows permuted", **kw)
    done(b, mats)


def test_the_form_the_stream_and_the_grid_change_no_bit(torch_cuda, tmp_path):
    torch = torch_cuda
    x, y, w, cuts, ev, want = DS.restated(4097, 4097, 12, 255, 1.0, 0.0, 0.5, 0.67, 9, rounds=2, weighted=True, held_out=1300)
    ex, _, ey, ew = ev
    kw = dict(rounds=2, max_depth=12, eta=0.5, reg_lambda=1.0, min_child_weight=0.0, subsample=0.5, colsample_bytree=0.67, seed=9)
    first = None
    for what, grid, device in (("plain", False, False), ("a grid said", True, False), ("device form on a stream", False, True),
                               ("device form, grid said", True, True)):
        b = capi.Booster(model_buffer=model())
        if device:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                tx, ty, tw = (torch.from_numpy(a).to("cuda") for a in (x, y, w))
                tex, tey, tew = (torch.from_numpy(a).to("cuda") for a in (ex, ey, ew))
            s.synchronize()
            d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=4097, ncol=3, missing=NAN)
            ed = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=1300, ncol=3, missing=NAN)
        else:
            d, ed = capi.DMatrix(x, missing=NAN), capi.DMatrix(ex, missing=NAN)
        if grid:
            d.set_grid(17, 241, 0)
            ed.set_grid(13, 10, 0)
        if device:
            got = b.boost_trees_deep_sampled_device(d, ty.data_ptr(), 4097, cuts, weights_ptr=tw.data_ptr(),
                                                    eval_set=(ed, tey.data_ptr(), 1300, tew.data_ptr()), stream=s.cuda_stream, **kw)
        else:
            got = b.boost_trees_deep_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **kw)
        same_result(got, want, what)
        same_new_trees(held(b, tmp_path)[0], want["trees"], 0, what)
        image = saved(b, tmp_path)
        first = first or image
        assert image == first, what
        done(b, [d, ed])


def test_what_follows_a_success(torch_cuda, tmp_path):
    x, y, w, cuts, ev, want = DS.restated(4097, 4097, 12, 255, 1.0, 0.0, 0.5, 0.67, 9, rounds=2)
    kw = dict(rounds=2, max_depth=12, eta=0.5, reg_lambda=1.0, min_child_weight=0.0, subsample=0.5, colsample_bytree=0.67, seed=9)
    got, b, (d,) = run(tmp_path, want, x, NAN, y, None, cuts, 3, what="first call", **kw)
    # margins by every kernel equal the restated running margin: every row moved, in or out of the bag
    for kernel, split in (("auto", "auto"), ("wide", "auto"), ("ring", "off")):
        b.set_param("ohx_kernel", kernel)
        b.set_param("ohx_tree_split", split)
        assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want["pred"])), kernel
    b.set_param("ohx_kernel", "auto")
    b.set_param("ohx_tree_split", "auto")
    # contributions run and add up
    dx = capi.DMatrix(x[:96], missing=NAN)
    m = b.predict(dx, option_mask=1).astype(np.float64)
    for approximate in (False, True):
        phi = b.predict_contribs(dx, approximate=approximate).astype(np.float64)
        assert np.all(np.abs(phi.sum(axis=1) - m) <= 1e-5 * (1.0 + np.abs(phi).sum(axis=1))), approximate
    # a visit count of all rows walks the new trees: the root sees every row, the bag's sum_hess only the bag
    b.count_visits(d)
    counts, seen = b.visit_counts()
    assert seen == 4097 and len(counts) == 2
    for c, t, bag in zip(counts, want["trees"], want["bags"]):
        assert int(c[0]) == 4097 > int(bag.sum()) == int(t["sum_hess"][0])
        inner = t["left"] >= 0
        assert np.array_equal(c[inner], c[t["left"][inner]] + c[t["right"][inner]]), "a node's rows are its children's"
    done(b, [d, dx])


def test_refusals_leave_the_model_unchanged_and_a_valid_call_follows(torch_cuda, tmp_path):
    torch = torch_cuda
    x, y, w, cuts, ev, want = DS.restated(4097, 4097, 12, 255, 1.0, 0.0, 0.5, 0.67, 9, rounds=2)
    kw = dict(rounds=2, max_depth=12, eta=0.5, reg_lambda=1.0, min_child_weight=0.0, subsample=0.5, colsample_bytree=0.67, seed=9)
    b = capi.Booster(model_buffer=model())
    d = capi.DMatrix(x, missing=NAN)
    before = saved(b, tmp_path)

    def valid(what):
        assert saved(b, tmp_path) == before, what
        same_result(b.boost_trees_deep_sampled(d, y, cuts, **kw), want, what)
        same_new_trees(held(b, tmp_path)[0], want["trees"], 0, what)
        b.load_model_buffer(model())

    # a NaN label on a row outside both bags is still a label refused
    out_row = int(np.flatnonzero(~want["bags"][0] & ~want["bags"][1])[0])
    yb = y.copy()
    yb[out_row] = np.nan
    with pytest.raises(ValueError, match="^label"):
        restate(x, NAN, yb, None, cuts, 3, **kw)
    with pytest.raises(capi.OhxError, match="a gradient pred - label") as err:
        b.boost_trees_deep_sampled(d, yb, cuts, **kw)
    assert "OHXBoosterBoostTreesDeepSampled" in str(err.value) and "unchanged" in str(err.value)
    valid("a NaN label on an out-of-bag row")
    # a bag without weight in the second round: its rows weigh nothing, the first bag's other rows do
    wb = np.ones(4097, np.float32)
    wb[want["bags"][1]] = 0.0
    assert np.count_nonzero(want["bags"][0] & ~want["bags"][1]) > 500
    with pytest.raises(ValueError, match="^bag"):
        restate(x, NAN, y, wb, cuts, 3, **kw)
    with pytest.raises(capi.OhxError, match="bag") as err:
        b.boost_trees_deep_sampled(d, y, cuts, weights=wb, **kw)
    assert "unchanged" in str(err.value)
    valid("a bag without weight in the second round")
    for bad in (dict(subsample=0.0), dict(subsample=1.5), dict(colsample_bytree=NAN), dict(colsample_bytree=-0.5)):
        with pytest.raises(capi.OhxError, match="subsample|colsample_bytree"):
            b.boost_trees_deep_sampled(d, y, cuts, **dict(kw, **bad))
    valid("fractions out of range")
    with pytest.raises(capi.OhxError, match=r"max_depth must be in 1\.\.18"):
        b.boost_trees_deep_sampled(d, y, cuts, **dict(kw, max_depth=19))
    valid("depth 19")
    # a stream that is being captured
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    dd = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=4097, ncol=3, missing=NAN)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="stream capture"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.boost_trees_deep_sampled_device(dd, ty.data_ptr(), 4097, cuts, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert saved(b, tmp_path) == before, "a captured stream"
    with torch.cuda.stream(s):
        got = b.boost_trees_deep_sampled_device(dd, ty.data_ptr(), 4097, cuts, stream=s.cuda_stream, **kw)
    same_result(got, want, "after the capture")
    done(b, [d, dd])
