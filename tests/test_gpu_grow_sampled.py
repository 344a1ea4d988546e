"""Boosting with row and column subsampling on the GPU (csrc/grow_sampled.hip, OHXBoosterBoostTreesSampled).  Every array
of every new tree, nodes_added, rounds_run and best_round are compared as integers or bit for bit, both RMSE arrays with
==, and models byte for byte.

Two kinds of expected values, neither from the code under test: the Weighted call on a twin booster (subsample and
colsample_bytree of 1 against the plain Weighted call; one sampled round against the Weighted call given the bag as 0 / 1
weights and the cuts of the unselected features emptied), and tests/grow_sampled_support.py, which restates the draws
and the call from include/ohxgb.h.  The margins a restatement starts from are margin predicts of a FRESH booster of the
same model, as in tests/test_gpu_grow.py."""
import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests import helpers
from tests.test_gpu_grow import base_model, level_sizes, margin_of, nfeat_of, same_new_trees, held
from tests.test_gpu_grow_eval import same_result, saved
from tests.test_gpu_grow_weighted import case, weights
from tests.test_grow_eval_cpu import early_stopping_case

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def ntrees(js):
    return len(G.trees_of(synth.convert_model(js, "json")))


def restate(js, x, missing, y, w, cuts, ev=None, **kw):
    """ev: (rows, missing, labels, weights or None).  Keyword names as the Python binding's; the forest of `js` gives T0."""
    pk = {"rounds": kw.get("rounds", 1), "max_depth": kw.get("max_depth", 6), "eta": kw.get("eta", 0.3),
          "lam": kw.get("reg_lambda", 1.0), "gamma": kw.get("gamma", 0.0),
          "min_child_weight": kw.get("min_child_weight", 1.0), "patience": kw.get("patience", 0),
          "subsample": kw.get("subsample", 1.0), "colsample_bytree": kw.get("colsample_bytree", 1.0), "seed": kw.get("seed", 0)}
    ep = margin_of(js, ev[0], ev[1]) if ev is not None else None
    return P.boost_sampled(margin_of(js, x, missing), x, missing, y, w, cuts, nfeat_of(js), eval_set=ev, eval_pred=ep,
                           tree0=ntrees(js), **pk)


def check(tmp_path, js, x, missing, y, w, cuts, ev=None, what="", **kw):
    """One host-form call on a fresh booster against the restatement -> (the restatement, the result, the booster)."""
    want = restate(js, x, missing, y, w, cuts, ev, **kw)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=missing)
    ed = capi.DMatrix(ev[0], missing=ev[1]) if ev is not None else None
    got = b.boost_trees_sampled(d, y, cuts, weights=w, eval_set=(ed, ev[2], ev[3]) if ev is not None else None, **kw)
    same_result(got, want, what)
    same_new_trees(held(b, tmp_path)[0], want["trees"], ntrees(js), what)
    d.free()
    if ed is not None:
        ed.free()
    return want, got, b


# ---- against the Weighted call: no restatement of the trees involved ----

@pytest.mark.parametrize("seed", (0, 7))
def test_all_rows_and_all_features_leave_what_the_weighted_call_leaves(torch_cuda, tmp_path, seed):
    js, x, y, ex, ey, cuts = case(27, 1000, 300, missing=-999.0)
    w, ew = weights(1, 1000), weights(2, 300)
    kw = dict(rounds=3, max_depth=5, eta=0.5, min_child_weight=0.5, patience=2)
    d = capi.DMatrix(x, missing=-999.0)
    ed = capi.DMatrix(ex, missing=NAN)
    twin = capi.Booster(model_buffer=js)
    want = twin.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **kw)
    b = capi.Booster(model_buffer=js)
    got = b.boost_trees_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, ew), subsample=1.0, colsample_bytree=1.0, seed=seed, **kw)
    assert got["train_rmse"].tolist() == want["train_rmse"].tolist()
    assert got["eval_rmse"].tolist() == want["eval_rmse"].tolist()
    assert (got["nodes_added"], got["rounds_run"], got["best_round"]) == (want["nodes_added"], want["rounds_run"], want["best_round"])
    assert saved(b, tmp_path) == saved(twin, tmp_path)
    for m in (d, ed):
        m.free()
    for bb in (b, twin):
        bb.free()


@pytest.mark.parametrize("subsample,colsample", [(0.5, 0.5), (0.7, 1.0), (1.0, 0.3)])
def test_one_round_is_the_weighted_call_with_the_bag_as_weights_and_emptied_cuts(torch_cuda, tmp_path, subsample, colsample):
    js, x, y, _, _, cuts = case(27, 1500, 1, missing=-999.0)
    w = weights(3, 1500)
    T0, seed = ntrees(js), 11
    mask = P.bag(seed, T0, 1500, subsample)
    kept = P.features(seed, T0, 27, colsample)
    assert (subsample == 1.0) == bool(mask.all()) and len(kept) == P.num_selected(27, colsample)
    kw = dict(rounds=1, max_depth=6, eta=0.5, min_child_weight=0.5)
    d = capi.DMatrix(x, missing=-999.0)
    twin = capi.Booster(model_buffer=js)
    want = twin.boost_trees_weighted(d, y, P.emptied_cuts(cuts, 27, kept), weights=(w * mask).astype(np.float32), **kw)
    b = capi.Booster(model_buffer=js)
    got = b.boost_trees_sampled(d, y, cuts, weights=w, subsample=subsample, colsample_bytree=colsample, seed=seed, **kw)
    assert got["nodes_added"] == want["nodes_added"] > 7
    assert saved(b, tmp_path) == saved(twin, tmp_path)
    d.free()
    for bb in (b, twin):
        bb.free()


# ---- against the restatement ----

@pytest.mark.parametrize("nfeat", (1, 3, 27))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_trees_and_both_rmse_arrays_equal_the_restatement(torch_cuda, tmp_path, n, nfeat):
    missing = -999.0 if (n + nfeat) % 2 else NAN
    ne = {1: 65, 63: 1, 64: 63, 65: 4097, 4097: 64}[n]
    js, x, y, ex, ey, cuts = case(nfeat, n, ne, missing=missing, emissing=missing)
    # one row: a seed whose first bag holds it (the empty bag is among the refusals)
    seed = next(s for s in range(n, n + 64) if n > 1 or P.bag(s, ntrees(js), 1, 0.6)[0] and P.bag(s, ntrees(js) + 1, 1, 0.6)[0])
    want, got, b = check(tmp_path, js, x, missing, y, None, cuts, (ex, missing, ey, None), f"{n} rows, {nfeat} features",
                         rounds=2, max_depth=6, eta=0.5, min_child_weight=0.5, subsample=0.6, colsample_bytree=0.5, seed=seed)
    assert all(len(f) == max(1, nfeat // 2) for f in want["features"])
    if n >= 63:
        assert all(0 < m.sum() < n for m in want["bags"]) and not np.array_equal(want["bags"][0], want["bags"][1])
    if n >= 4097:
        assert len(want["trees"][0]["left"]) > 15 and want["train_rmse"][-1] < want["train_rmse"][0]
        used = [set(t["feature"][t["left"] >= 0].tolist()) for t in want["trees"]]
        assert all(u <= set(f) for u, f in zip(used, want["features"]))
    b.free()


@pytest.mark.parametrize("max_depth,rounds", [(1, 5), (2, 2), (6, 1), (8, 2)])
def test_depths_and_rounds(torch_cuda, tmp_path, max_depth, rounds):
    js, x, y, ex, ey, _ = case(3, 4097, 500, missing=-999.0)
    cuts = capi.quantile_cuts(x, -999.0, 255)
    want, got, b = check(tmp_path, js, x, -999.0, y, None, cuts, (ex, NAN, ey, None), f"depth {max_depth}", rounds=rounds,
                         max_depth=max_depth, eta=0.5, min_child_weight=0.0, subsample=0.75, colsample_bytree=0.67, seed=max_depth + 9)
    assert all(len(t["left"]) <= 2 ** (max_depth + 1) - 1 for t in want["trees"]) and all(len(f) == 2 for f in want["features"])
    if max_depth == 8:
        assert max(max(level_sizes(t)[:8]) for t in want["trees"]) > 40, "a level of more than 40 open nodes"
    if rounds == 5:
        assert len({tuple(f) for f in want["features"]}) > 1, "the rounds draw different features"
    b.free()


@pytest.mark.parametrize("colsample", (0.5, 0.3))
def test_128_features_at_depth_8_where_n_sel_is_no_multiple_of_a_feature_group(torch_cuda, tmp_path, colsample):
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, F = 4097, 128
    p = synth.grow_plan_sampled(n, F, colsample, 0, 8, cus)
    n_sel = p["n_sel"]
    assert n_sel == {0.5: 64, 0.3: 38}[colsample]
    assert any(n_sel % l["feat_group"] != 0 for l in p["levels"]), "a last feature group that is not full"
    assert p["levels"][7]["node_groups"] >= 2 and p["levels"][7]["feat_groups"] >= 2 and p["levels"][2]["feat_groups"] >= 2
    js = base_model(F, 2)
    rng = np.random.default_rng(128)
    x = rng.normal(0, 1, (n, F)).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    y = (margin_of(js, x, NAN) + np.nan_to_num(x[:, 5] * x[:, 100]) + np.nan_to_num(x[:, 127]) + np.nan_to_num(x[:, :64]).sum(axis=1) * 0.05).astype(np.float32)
    want, got, b = check(tmp_path, js, x, NAN, y, None, capi.quantile_cuts(x, NAN, 8), None, "128 features", max_depth=8,
                         eta=0.3, min_child_weight=2.0, subsample=0.9, colsample_bytree=colsample, seed=128)
    assert max(level_sizes(want["trees"][0])[:8]) > 40, "more open nodes at a level than one block holds"
    used = set(want["trees"][0]["feature"][want["trees"][0]["left"] >= 0].tolist())
    assert used <= set(want["features"][0]) and max(used) > 64 and len(used) > 10
    b.free()


def test_weights_mixed_with_sampling_and_a_zero_weight_row_in_the_bag(torch_cuda, tmp_path):
    js, x, y, ex, ey, cuts = case(3, 1000, 300)
    w, ew = weights(50, 1000), weights(51, 300)
    seed = 5
    mask = P.bag(seed, ntrees(js), 1000, 0.5)
    assert (w[mask] == 0).any() and (w[~mask] == 0).any() and (w[mask] > 0).any(), "zero-weight rows in the bag and out of it"
    want, got, b = check(tmp_path, js, x, NAN, y, w, cuts, (ex, NAN, ey, ew), "weights and sampling", rounds=3, max_depth=5,
                         eta=0.5, min_child_weight=0.25, subsample=0.5, colsample_bytree=0.67, seed=seed)
    # sum_hess of the root is the bag's weight, and the training W every row's
    assert want["trees"][0]["sum_hess"][0] == np.float32(P.W.hess(P.W.hess_fixed(w[mask]).astype(object).sum()))
    assert want["train_W"] == int(P.W.hess_fixed(w).astype(object).sum())
    b.free()


def test_more_rows_than_two_trips_of_every_new_kernels_loop(torch_cuda, tmp_path):
    """The bag kernel strides over row_blocks x 256 rows and the histogram kernel over hist_blocks x 1024; the row count is
    no multiple of 64, so the last word of the bit plane has a tail."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = synth.grow_plan_sampled(1 << 30, 2, 1.0, 10, 2, cus)
    trip = max(full["row_blocks"] * full["block_rows"], max(l["hist_blocks"] for l in full["levels"]) * full["hist_block_rows"])
    n = 2 * trip + 77
    p = synth.grow_plan_sampled(n, 2, 1.0, 10, 2, cus)
    assert n % 64 != 0 and all(n > 2 * l["hist_blocks"] * p["hist_block_rows"] for l in p["levels"]) and n > 2 * p["row_blocks"] * 256
    js = base_model(2, 1)
    rng = np.random.default_rng(9)
    x = np.empty((n, 2), dtype=np.float32)
    x[:, 0] = rng.integers(0, 10, n)
    x[:, 1] = rng.integers(0, 2, n)
    x[rng.random(n) < 0.01, 0] = np.nan
    cuts = capi.quantile_cuts(x[:5000], NAN)
    y = (margin_of(js, x, NAN) + np.nan_to_num(x[:, 0]) * 0.1 - x[:, 1] + rng.normal(0, 0.1, n)).astype(np.float32)
    want, got, b = check(tmp_path, js, x, NAN, y, None, cuts, None, "past the launch caps", max_depth=2, eta=0.5,
                         subsample=0.5, seed=3)
    assert len(want["trees"][0]["left"]) == 7 and abs(want["bags"][0].mean() - 0.5) < 0.005
    # the tail of the plane is clear: the last rows of the bag are the restatement's, none past them adds
    assert want["trees"][0]["sum_hess"][0] == np.float32(want["bags"][0].sum())
    b.free()


def test_the_order_of_the_rows_enters_through_the_draw_alone(torch_cuda, tmp_path):
    js, x, y, _, _, cuts = case(3, 1200, 1)
    kw = dict(rounds=2, max_depth=5, eta=0.5, subsample=0.5, colsample_bytree=0.67, seed=21)
    perm = np.random.default_rng(1).permutation(1200)
    xp, yp = np.ascontiguousarray(x[perm]), y[perm].copy()
    plain, _, b = check(tmp_path, js, x, NAN, y, None, cuts, None, "plain", **kw)
    image = saved(b, tmp_path)
    b.free()
    permuted, _, b = check(tmp_path, js, xp, NAN, yp, None, cuts, None, "rows permuted", **kw)
    assert saved(b, tmp_path) != image, "row r of the permuted matrix is another row: another bag, another forest"
    assert permuted["train_rmse"] != plain["train_rmse"]
    b.free()
    # without row sampling the order of the rows changes nothing (the features do not depend on it)
    kw["subsample"] = 1.0
    _, _, b = check(tmp_path, js, x, NAN, y, None, cuts, None, "columns only", **kw)
    _, _, bp = check(tmp_path, js, xp, NAN, yp, None, cuts, None, "columns only, permuted", **kw)
    assert saved(b, tmp_path) == saved(bp, tmp_path)
    for bb in (b, bp):
        bb.free()


def test_the_form_the_stream_and_the_grid_change_no_bit(torch_cuda, tmp_path):
    torch = torch_cuda
    js, x, y, ex, ey, cuts = case(27, 1200, 1300, missing=-999.0, emissing=-999.0)
    w, ew = weights(20, 1200), weights(21, 1300)
    kw = dict(rounds=3, max_depth=5, eta=0.5, patience=2, min_child_weight=0.25, subsample=0.6, colsample_bytree=0.5, seed=77)
    want = restate(js, x, -999.0, y, w, cuts, (ex, -999.0, ey, ew), **kw)
    first = None
    for what, grid, device in (("plain", None, "host"), ("a grid said", (13, 10, 0), "host"),
                               ("device form on a stream", None, "device"), ("device form, grid said", (13, 10, 0), "device"),
                               ("a device held-out matrix in the host form", None, "mixed")):
        b = capi.Booster(model_buffer=js)
        if device != "host":
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                tx, ty, tw = (torch.from_numpy(a).to("cuda") for a in (x, y, w))
                tex, tey, tew = (torch.from_numpy(a).to("cuda") for a in (ex, ey, ew))
            s.synchronize()
        d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=1200, ncol=27, missing=-999.0) if device == "device" else capi.DMatrix(x, missing=-999.0)
        ed = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=1300, ncol=27, missing=-999.0) if device != "host" else capi.DMatrix(ex, missing=-999.0)
        if grid is not None:
            d.set_grid(12, 10, 0)
            ed.set_grid(*grid)
        if device == "device":
            got = b.boost_trees_sampled_device(d, ty.data_ptr(), 1200, cuts, weights_ptr=tw.data_ptr(),
                                               eval_set=(ed, tey.data_ptr(), 1300, tew.data_ptr()), stream=s.cuda_stream, **kw)
        else:
            got = b.boost_trees_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **kw)
        same_result(got, want, what)
        same_new_trees(held(b, tmp_path)[0], want["trees"], 3, what)
        image = saved(b, tmp_path)
        first = first or image
        assert image == first, what
        for m in (d, ed):
            m.free()
        b.free()


def test_the_trees_the_forest_holds_move_the_draw(torch_cuda, tmp_path):
    """T0 = 0, T0 = 3, and a second call on the same booster (T0 = 3 + 2): each restated from the forest it starts from."""
    x = None
    for ntree in (0, 3):
        js = base_model(3, ntree)
        _, x, y, _, _, cuts = case(3, 800, 1, ntree=ntree)
        kw = dict(rounds=2, max_depth=4, eta=0.5, subsample=0.5, colsample_bytree=0.67, seed=9)
        want, got, b = check(tmp_path, js, x, NAN, y, None, cuts, None, f"T0 = {ntree}", **kw)
        assert [m.tolist() for m in want["bags"]] == [P.bag(9, ntree + r, 800, 0.5).tolist() for r in range(2)]
        if ntree == 3:
            # the second call draws trees 5 and 6
            js2 = held(b, tmp_path)[1]
            assert ntrees(js2) == 5
            want2 = restate(js2, x, NAN, y, None, cuts, None, **kw)
            assert not np.array_equal(want2["bags"][0], want["bags"][0])
            d = capi.DMatrix(x, missing=NAN)
            got2 = b.boost_trees_sampled(d, y, cuts, **kw)
            same_result(got2, want2, "the second call")
            same_new_trees(held(b, tmp_path)[0], want2["trees"], 5, "the second call")
            d.free()
        b.free()


def test_early_stopping_with_the_best_round_strictly_inside_and_what_follows_a_success(torch_cuda, tmp_path):
    xt, yt, xe, ye, cuts = early_stopping_case()
    js = G.empty_model(3, base=0.0)
    kw = dict(rounds=20, max_depth=6, eta=0.5, reg_lambda=1.0, patience=3, min_child_weight=1.0, subsample=0.8,
              colsample_bytree=0.67, seed=1)
    want = restate(js, xt, NAN, yt, None, cuts, (xe, NAN, ye, None), **kw)
    assert 0 < want["best_round"] < want["rounds_run"] < 20
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(xt, missing=NAN)
    ed = capi.DMatrix(xe, missing=NAN)
    got = b.boost_trees_sampled(d, yt, cuts, eval_set=(ed, ye), **kw)
    same_result(got, want, "early stopping")
    assert len(got["eval_rmse"]) == want["rounds_run"] + 1
    same_new_trees(held(b, tmp_path)[0], want["trees"], 0, "early stopping")
    # after a success: the truncated forest predicts by every kernel, and contributions work
    for kernel, split in (("auto", "auto"), ("wide", "auto"), ("ring", "off")):
        b.set_param("ohx_kernel", kernel)
        b.set_param("ohx_tree_split", split)
        assert np.array_equal(helpers.bits(b.predict(ed, option_mask=1)), helpers.bits(want["eval_pred"])), kernel
        assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want["pred"])), kernel
    dx = capi.DMatrix(xe[:96], missing=NAN)
    m = b.predict(dx, option_mask=1).astype(np.float64)
    phi = b.predict_contribs(dx).astype(np.float64)
    assert np.all(np.abs(phi.sum(axis=1) - m) <= 1e-5 * (1.0 + np.abs(phi).sum(axis=1)))
    for mtx in (d, ed, dx):
        mtx.free()
    b.free()


# ---- refusals on the GPU ----

def test_refusals_leave_the_model_unchanged_and_a_valid_call_follows(torch_cuda, tmp_path):
    torch = torch_cuda
    js, x, y, ex, ey, cuts = case(3, 1000, 300)
    w, ew = weights(40, 1000), weights(41, 300)
    kw = dict(rounds=2, max_depth=3, patience=1, subsample=0.5, colsample_bytree=0.67, seed=4)
    ev = (ex, NAN, ey, ew)
    want = restate(js, x, NAN, y, w, cuts, ev, **kw)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=NAN)
    ed = capi.DMatrix(ex, missing=NAN)
    before = saved(b, tmp_path)

    def valid(what):
        assert saved(b, tmp_path) == before, what
        same_result(b.boost_trees_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **kw), want, what)
        b.load_model_buffer(js)

    mask = P.bag(4, 3, 1000, 0.5)
    out_row, in_row = int(np.flatnonzero(~mask)[0]), int(np.flatnonzero(mask)[0])
    # a bad weight, in the bag or out of it: the weight refusals cover all rows
    for row in (in_row, out_row):
        wb = w.copy()
        wb[row] = np.nan
        with pytest.raises(ValueError, match="^weight"):
            restate(js, x, NAN, y, wb, cuts, ev, **kw)
        with pytest.raises(capi.OhxError, match="a weight is not finite"):
            b.boost_trees_sampled(d, y, cuts, weights=wb, eval_set=(ed, ey, ew), **kw)
        valid(f"a NaN weight at row {row}")
    # a NaN label on an out-of-bag row is still a label refused
    yb = y.copy()
    yb[out_row] = np.nan
    with pytest.raises(ValueError, match="^label"):
        restate(js, x, NAN, yb, w, cuts, ev, **kw)
    with pytest.raises(capi.OhxError, match="a gradient pred - label") as err:
        b.boost_trees_sampled(d, yb, cuts, weights=w, eval_set=(ed, ey, ew), **kw)
    assert "eval label" not in str(err.value) and "unchanged" in str(err.value)
    valid("a NaN label on an out-of-bag row")
    # an eval weight
    eb = ew.copy()
    eb[299] = -1.0
    with pytest.raises(capi.OhxError, match="eval weight"):
        b.boost_trees_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, eb), **kw)
    valid("an eval weight of -1")
    # a bag without weight: every row of the first bag weighs nothing
    wb = w.copy()
    wb[mask] = 0.0
    with pytest.raises(ValueError, match="^bag"):
        restate(js, x, NAN, y, wb, cuts, ev, **kw)
    with pytest.raises(capi.OhxError, match="bag") as err:
        b.boost_trees_sampled(d, y, cuts, weights=wb, eval_set=(ed, ey, ew), **kw)
    assert "unchanged" in str(err.value)
    valid("a bag whose rows weigh nothing")
    # an empty bag: one row, and a seed for which tree T0 = 3 does not draw it
    assert not P.bag(0, 3, 1, 0.5)[0] and P.bag(2, 3, 1, 0.5)[0]
    d1 = capi.DMatrix(x[:1], missing=NAN)
    one = dict(rounds=1, max_depth=3, subsample=0.5)
    with pytest.raises(ValueError, match="^bag"):
        restate(js, x[:1], NAN, y[:1], None, cuts, None, seed=0, **one)
    with pytest.raises(capi.OhxError, match="bag"):
        b.boost_trees_sampled(d1, y[:1], cuts, seed=0, **one)
    assert saved(b, tmp_path) == before, "an empty bag"
    same_result(b.boost_trees_sampled(d1, y[:1], cuts, seed=2, **one), restate(js, x[:1], NAN, y[:1], None, cuts, None, seed=2, **one),
                "one row that is drawn")
    b.load_model_buffer(js)
    # ... also in the second round, whether the stop rule would have kept its tree or not (patience 2 runs both rounds)
    seed = next(s for s in range(100) if P.bag(s, 3, 1, 0.5)[0] and not P.bag(s, 4, 1, 0.5)[0])
    with pytest.raises(ValueError, match="^bag"):
        restate(js, x[:1], NAN, y[:1], None, cuts, (ex, NAN, ey, None), rounds=2, max_depth=3, subsample=0.5, seed=seed, patience=2)
    with pytest.raises(capi.OhxError, match="bag"):
        b.boost_trees_sampled(d1, y[:1], cuts, eval_set=(ed, ey), rounds=2, max_depth=3, subsample=0.5, seed=seed, patience=2)
    valid("an empty bag in the second round")
    # the refusals that need no device, with a matrix at hand
    for bad in (dict(subsample=0.0), dict(subsample=1.5), dict(colsample_bytree=float("nan")), dict(colsample_bytree=-0.5)):
        with pytest.raises(capi.OhxError, match="subsample|colsample_bytree"):
            b.boost_trees_sampled(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **dict(kw, **bad))
    valid("bad fractions")
    # a stream that is being captured
    tx, ty, tw = (torch.from_numpy(a).cuda() for a in (x, y, w))
    tex, tey, tew = (torch.from_numpy(a).cuda() for a in (ex, ey, ew))
    dd = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=1000, ncol=3, missing=NAN)
    de = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=300, ncol=3, missing=NAN)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="stream capture"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.boost_trees_sampled_device(dd, ty.data_ptr(), 1000, cuts, weights_ptr=tw.data_ptr(),
                                         eval_set=(de, tey.data_ptr(), 300, tew.data_ptr()),
                                         stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert saved(b, tmp_path) == before, "a captured stream"
    with torch.cuda.stream(s):
        got = b.boost_trees_sampled_device(dd, ty.data_ptr(), 1000, cuts, weights_ptr=tw.data_ptr(),
                                           eval_set=(de, tey.data_ptr(), 300, tew.data_ptr()), stream=s.cuda_stream, **kw)
    same_result(got, want, "after the capture")
    for m in (d, ed, dd, de, d1):
        m.free()
    b.free()


# ---- the kinds of call in sequence on one handle ----

def test_the_four_kinds_in_sequence_on_one_handle_leave_what_fresh_boosters_leave(torch_cuda, tmp_path):
    """One booster takes a plain Device call, a Sampled, a Weighted, an Eval and a plain call again, 2 rounds each: the
    kinds share the handle's grow state - its one prepared flag and its buffers, sized by a different plan each time.
    After every step the saved bytes (all three formats) equal those of a fresh booster loaded from the previous
    step's UBJSON bytes and given that one call: save then load keeps every field bit for bit (the comparison itself
    would show a field that did not)."""
    torch = torch_cuda
    js, x, y, ex, ey, cuts = case(3, 4097, 65, missing=-999.0)
    w = weights(5, 4097)
    kw = dict(rounds=2, max_depth=3, eta=0.5)
    d = capi.DMatrix(x, missing=-999.0)
    ed = capi.DMatrix(ex, missing=NAN)
    yd = torch.from_numpy(y).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def plain_device(b):
        return b.boost_trees_device(d, yd.data_ptr(), y.size, cuts, stream=stream, **kw)

    steps = [("plain Device", plain_device),
             ("Sampled", lambda b: b.boost_trees_sampled(d, y, cuts, subsample=0.5, colsample_bytree=0.5, seed=3, **kw)),
             ("Weighted", lambda b: b.boost_trees_weighted(d, y, cuts, weights=w, **kw)),
             ("Eval", lambda b: b.boost_trees_eval(d, y, cuts, eval_set=(ed, ey), patience=0, **kw)),
             ("plain again", lambda b: b.boost_trees(d, y, cuts, **kw))]
    one = capi.Booster(model_buffer=js)
    before, trees = js, ntrees(js)
    for what, call in steps:
        got = call(one)
        twin = capi.Booster(model_buffer=before)
        want = call(twin)
        if isinstance(want, dict):
            assert (got["nodes_added"], got["rounds_run"], got["best_round"]) == (want["nodes_added"], 2, 2), what
            assert got["train_rmse"].tolist() == want["train_rmse"].tolist(), what
            if want["eval_rmse"] is not None:
                assert got["eval_rmse"].tolist() == want["eval_rmse"].tolist(), what
        else:
            assert got == want > 2, what
        after = saved(one, tmp_path)
        assert after == saved(twin, tmp_path), what
        twin.free()
        trees += 2
        assert ntrees(after[0]) == trees, what
        before = after[1]
    torch.cuda.synchronize()
    for m in (d, ed):
        m.free()
    one.free()
