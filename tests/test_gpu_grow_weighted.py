"""Boosting with row weights on the GPU (csrc/grow_weighted.hip, OHXBoosterBoostTreesWeighted).  Every array of every new
tree, nodes_added, rounds_run and best_round are compared as integers or bit for bit, both RMSE arrays with ==, and
models byte for byte.

Two kinds of expected values, neither from the code under test: the existing calls on a twin booster (unit weights
against OHXBoosterBoostTreesEval; weights 0 / 1 against the matrix without the zero-weight rows; weights 1 / 2 / 4 against
the matrix with rows repeated), and tests/grow_weighted_support.py, which restates the call from include/ohxgb.h.  The
margins a restatement starts from are margin predicts of a FRESH booster of the same model, as in tests/test_gpu_grow.py."""
import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_support as G
from tests import grow_weighted_support as W
from tests import helpers
from tests.test_gpu_grow import base_model, labels, level_sizes, margin_of, nfeat_of, rows, same_new_trees, held
from tests.test_gpu_grow_eval import same_result, saved
from tests.test_grow_eval_cpu import early_stopping_case

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def weights(seed, n, kind="random"):
    """random: uniform in [0, 4) as float32, mantissas below the 2^-24 fixed point's resolution, a tenth of them 0."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        w = (rng.random(n) * 4).astype(np.float32)
        w[rng.random(n) < 0.1] = 0.0
        if n > 1:
            w[0] = np.float32(2.0 ** -26)          # rint(w * 2^24) = 0 with a gradient that is not
            w[-1] = np.float32(1.0 + 2.0 ** -23)
        else:
            w[0] = np.float32(0.7)
        return w
    return rng.choice(np.asarray(kind, np.float32), n).astype(np.float32)


def restate(js, x, missing, y, w, cuts, ev=None, **kw):
    """ev: (rows, missing, labels, weights or None).  Keyword names as the Python binding's."""
    pk = {"rounds": kw.get("rounds", 1), "max_depth": kw.get("max_depth", 6), "eta": kw.get("eta", 0.3),
          "lam": kw.get("reg_lambda", 1.0), "gamma": kw.get("gamma", 0.0),
          "min_child_weight": kw.get("min_child_weight", 1.0), "patience": kw.get("patience", 0)}
    ep = margin_of(js, ev[0], ev[1]) if ev is not None else None
    return W.boost_weighted(margin_of(js, x, missing), x, missing, y, w, cuts, nfeat_of(js), eval_set=ev, eval_pred=ep, **pk)


def check(tmp_path, js, x, missing, y, w, cuts, ev=None, what="", grid=None, **kw):
    """One host-form call on a fresh booster against the restatement -> (the restatement, the result, the booster)."""
    want = restate(js, x, missing, y, w, cuts, ev, **kw)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=missing)
    if grid is not None:
        d.set_grid(*grid)
    ed = capi.DMatrix(ev[0], missing=ev[1]) if ev is not None else None
    got = b.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ev[2], ev[3]) if ev is not None else None, **kw)
    same_result(got, want, what)
    nold = len(G.trees_of(synth.convert_model(js, "json")))
    same_new_trees(held(b, tmp_path)[0], want["trees"], nold, what)
    d.free()
    if ed is not None:
        ed.free()
    return want, got, b


def case(nfeat, ntrain, neval, missing=NAN, emissing=NAN, seed=0, ntree=3, bins=64):
    js = base_model(nfeat, ntree)
    x = rows(seed + ntrain * 7 + nfeat, ntrain, nfeat, missing)
    y = labels(seed + ntrain, x, margin_of(js, x, missing))
    ex = rows(seed + neval * 11 + nfeat + 1, neval, nfeat, emissing)
    ey = labels(seed + neval + 1, ex, margin_of(js, ex, emissing))
    return js, x, y, ex, ey, capi.quantile_cuts(x, missing, bins)


# ---- against the existing calls: no restatement involved ----

@pytest.mark.parametrize("nfeat,max_depth,rounds", [(1, 1, 5), (3, 6, 2), (27, 8, 2)])
def test_unit_weights_leave_what_the_eval_call_leaves(torch_cuda, tmp_path, nfeat, max_depth, rounds):
    js, x, y, ex, ey, cuts = case(nfeat, 1000, 300, missing=-999.0)
    kw = dict(rounds=rounds, max_depth=max_depth, eta=0.5)
    d = capi.DMatrix(x, missing=-999.0)
    ed = capi.DMatrix(ex, missing=NAN)
    for mcr in (1, 7):
        twin = capi.Booster(model_buffer=js)
        want = twin.boost_trees_eval(d, y, cuts, eval_set=(ed, ey), min_child_rows=mcr, **kw)
        want_bytes = saved(twin, tmp_path)
        for what, w, ew in (("NULL", None, None), ("ones", np.ones(1000, np.float32), np.ones(300, np.float32)),
                            ("ones and NULL", np.ones(1000, np.float32), None)):
            b = capi.Booster(model_buffer=js)
            got = b.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ey, ew), min_child_weight=float(mcr), **kw)
            assert got["train_rmse"].tolist() == want["train_rmse"].tolist(), what
            assert got["eval_rmse"].tolist() == want["eval_rmse"].tolist(), what
            assert (got["nodes_added"], got["rounds_run"], got["best_round"]) == (want["nodes_added"], want["rounds_run"], want["best_round"])
            assert saved(b, tmp_path) == want_bytes, (what, mcr)
            b.free()
        twin.free()
    for m in (d, ed):
        m.free()


def test_zero_weight_rows_are_rows_that_are_not_there(torch_cuda, tmp_path):
    js, x, y, ex, ey, cuts = case(3, 1500, 700, missing=-999.0, emissing=-999.0)
    w = weights(1, 1500, (0.0, 1.0))
    ew = weights(2, 700, (0.0, 1.0))
    assert 0 < w.sum() < 1500 and 0 < ew.sum() < 700
    kw = dict(rounds=3, max_depth=5, eta=0.5)
    d = capi.DMatrix(x, missing=-999.0)
    ed = capi.DMatrix(ex, missing=-999.0)
    dk = capi.DMatrix(np.ascontiguousarray(x[w == 1]), missing=-999.0)
    ek = capi.DMatrix(np.ascontiguousarray(ex[ew == 1]), missing=-999.0)
    twin = capi.Booster(model_buffer=js)
    want = twin.boost_trees_eval(dk, y[w == 1], cuts, eval_set=(ek, ey[ew == 1]), min_child_rows=2, **kw)
    b = capi.Booster(model_buffer=js)
    got = b.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ey, ew), min_child_weight=2.0, **kw)
    assert saved(b, tmp_path) == saved(twin, tmp_path)
    assert got["train_rmse"].tolist() == want["train_rmse"].tolist()
    assert got["eval_rmse"].tolist() == want["eval_rmse"].tolist()
    assert got["nodes_added"] == want["nodes_added"]
    for m in (d, ed, dk, ek):
        m.free()
    for bb in (b, twin):
        bb.free()


def test_weights_1_2_4_are_that_many_copies_of_the_row(torch_cuda, tmp_path):
    """Residuals of 2 to 3 in size and eta 0.1 (a round moves a margin by 0.3 at most) keep every |g| >= 0.5 over the rounds, where g * 2^24 is a whole number and
    rint(w * x) = w * rint(x): the histograms of the copies are the weighted ones."""
    js = base_model(3)
    rng = np.random.default_rng(7)
    x = rows(71, 600, 3, NAN)
    ex = rows(72, 250, 3, NAN)
    z = np.nan_to_num(x[:, 0])
    y = (margin_of(js, x, NAN) + np.where(z > 0.2, 1.0, -1.0) * rng.uniform(2.0, 3.0, 600)).astype(np.float32)
    ey = (margin_of(js, ex, NAN) + np.where(np.nan_to_num(ex[:, 0]) > 0.2, 1.0, -1.0) * rng.uniform(2.0, 3.0, 250)).astype(np.float32)
    w = weights(3, 600, (1.0, 2.0, 4.0))
    ew = weights(4, 250, (1.0, 2.0, 4.0))
    cuts = capi.quantile_cuts(x, NAN, 32)
    kw = dict(rounds=3, max_depth=4, eta=0.1)
    want_r = restate(js, x, NAN, y, w, cuts, (ex, NAN, ey, ew), min_child_weight=3.0, **kw)
    assert all(np.abs(p - y).min() >= 0.5 for p in want_r["preds"]), "the premise: every |g| >= 0.5"
    rep, erep = np.repeat(np.arange(600), w.astype(int)), np.repeat(np.arange(250), ew.astype(int))
    d = capi.DMatrix(x, missing=NAN)
    ed = capi.DMatrix(ex, missing=NAN)
    dr = capi.DMatrix(np.ascontiguousarray(x[rep]), missing=NAN)
    er = capi.DMatrix(np.ascontiguousarray(ex[erep]), missing=NAN)
    twin = capi.Booster(model_buffer=js)
    want = twin.boost_trees_eval(dr, y[rep], cuts, eval_set=(er, ey[erep]), min_child_rows=3, **kw)
    b = capi.Booster(model_buffer=js)
    got = b.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ey, ew), min_child_weight=3.0, **kw)
    assert saved(b, tmp_path) == saved(twin, tmp_path)
    assert got["train_rmse"].tolist() == want["train_rmse"].tolist()
    assert got["eval_rmse"].tolist() == want["eval_rmse"].tolist()
    assert got["nodes_added"] == want["nodes_added"] > 3
    same_result(got, want_r, "and the restatement")
    for m in (d, ed, dr, er):
        m.free()
    for bb in (b, twin):
        bb.free()


# ---- against the restatement ----

@pytest.mark.parametrize("nfeat", (1, 3, 27))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_trees_and_both_rmse_arrays_equal_the_restatement(torch_cuda, tmp_path, n, nfeat):
    missing = -999.0 if (n + nfeat) % 2 else NAN
    ne = {1: 65, 63: 1, 64: 63, 65: 4097, 4097: 64}[n]
    js, x, y, ex, ey, cuts = case(nfeat, n, ne, missing=missing, emissing=missing)
    w, ew = weights(n, n), weights(n + 1, ne)
    want, got, b = check(tmp_path, js, x, missing, y, w, cuts, (ex, missing, ey, ew), f"{n} rows, {nfeat} features",
                         rounds=2, max_depth=6, eta=0.5, min_child_weight=0.5)
    if n >= 4097:
        assert len(want["trees"][0]["left"]) > 15 and want["train_rmse"][-1] < want["train_rmse"][0]
    b.free()


@pytest.mark.parametrize("max_depth,rounds", [(1, 5), (2, 2), (6, 1), (8, 2)])
def test_depths_and_rounds(torch_cuda, tmp_path, max_depth, rounds):
    js, x, y, ex, ey, _ = case(3, 4097, 500, missing=-999.0)
    cuts = capi.quantile_cuts(x, -999.0, 255)
    want, got, b = check(tmp_path, js, x, -999.0, y, weights(5, 4097), cuts, (ex, NAN, ey, weights(6, 500)), f"depth {max_depth}",
                         rounds=rounds, max_depth=max_depth, eta=0.5, min_child_weight=0.0)
    assert all(len(t["left"]) <= 2 ** (max_depth + 1) - 1 for t in want["trees"])
    if max_depth == 8:
        assert max(max(level_sizes(t)[:8]) for t in want["trees"]) > 40, "a level of more than 40 open nodes"
    b.free()


def test_128_features_at_depth_8_take_several_node_and_feature_groups(torch_cuda, tmp_path):
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, F = 4097, 128
    p = synth.grow_plan_weighted(n, F, 0, 8, cus)
    assert p["levels"][7]["node_groups"] >= 2 and p["levels"][7]["feat_groups"] >= 2 and p["levels"][0]["feat_groups"] >= 2
    assert all(l["node_group"] * l["feat_group"] <= 40 for l in p["levels"])
    js = base_model(F, 2)
    rng = np.random.default_rng(128)
    x = rng.normal(0, 1, (n, F)).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    y = (margin_of(js, x, NAN) + np.nan_to_num(x[:, 5] * x[:, 100]) + np.nan_to_num(x[:, 127])).astype(np.float32)
    want, got, b = check(tmp_path, js, x, NAN, y, weights(128, n), capi.quantile_cuts(x, NAN, 8), None, "128 features",
                         max_depth=8, eta=0.3, min_child_weight=4.0)
    assert max(level_sizes(want["trees"][0])[:8]) > 40, "more open nodes at a level than one block holds"
    b.free()


def test_weights_at_the_edge_an_empty_side_of_every_cut_lambda_zero_and_fewer_columns(torch_cuda, tmp_path):
    """Weights of 256 - 2^-16 on rows whose |g| < 0.5; column 0 has one cut and every row below it weighs nothing, so HL == 0
    at its only candidates and lambda = 0 would divide by zero; the matrix holds three of the booster's five features."""
    n, F = 1000, 5
    js = base_model(F)
    rng = np.random.default_rng(11)
    x = rows(11, n, 3, NAN)
    x[:, 0] = rng.integers(0, 2, n)
    cuts3 = capi.quantile_cuts(x, NAN, 32)
    assert cuts3[0][1] == 1
    cuts = (np.concatenate([cuts3[0], cuts3[0][-1:], cuts3[0][-1:]]), cuts3[1])
    m = margin_of(js, x, NAN)
    y = labels(5, x, m, scale=0.3)
    w = weights(12, n)
    edge = np.float32(256.0 - 2.0 ** -16)
    big = np.flatnonzero((np.abs(m - y) < 0.5) & (x[:, 0] == 1))[:20]
    assert len(big) == 20
    w[big] = edge
    w[x[:, 0] == 0] = 0.0
    assert int(W.hess_fixed(w[big[:1]])[0]) == (1 << 32) - 256
    want, got, b = check(tmp_path, js, x, NAN, y, w, cuts, (x, NAN, y, w), "edges", rounds=2, max_depth=4, eta=0.5,
                         reg_lambda=0.0, min_child_weight=0.0)
    used = np.concatenate([t["feature"][t["left"] >= 0] for t in want["trees"]])
    assert len(used) > 2 and 0 not in used and (used < 3).all()
    assert not np.isnan(got["train_rmse"]).any() and got["eval_rmse"].tolist() == got["train_rmse"].tolist()
    assert all(np.isfinite(t["value"]).all() for t in want["trees"])
    b.free()


def test_a_min_child_weight_that_forbids_every_split(torch_cuda, tmp_path):
    js, x, y, _, _, cuts = case(3, 200, 1)
    w = weights(13, 200)
    total = float(W.hess(W.hess_fixed(w).astype(object).sum()))
    want, got, b = check(tmp_path, js, x, NAN, y, w, cuts, None, "more than half the weight", min_child_weight=total * 0.51)
    assert len(want["trees"][0]["left"]) == 1 and want["trees"][0]["value"][0] != 0.0
    assert want["trees"][0]["sum_hess"][0] == np.float32(total)
    b.free()
    want, got, b = check(tmp_path, js, x, NAN, y, w, cuts, None, "one split at most per path", min_child_weight=total * 0.36, max_depth=4)
    assert len(want["trees"][0]["left"]) == 3
    b.free()


def test_more_rows_than_two_trips_of_every_new_kernels_loop(torch_cuda, tmp_path):
    """The training set is held out as well, so the walk kernel strides too.  The trips come from the exported plans."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = synth.grow_plan_weighted(1 << 30, 2, 10, 2, cus)
    trip = max(full["row_blocks"] * full["block_rows"], max(l["hist_blocks"] for l in full["levels"]) * full["hist_block_rows"],
               synth.grow_eval_plan(1 << 30, cus)["blocks"] * 256)
    n = 2 * trip + 77
    p = synth.grow_plan_weighted(n, 2, 10, 2, cus)
    assert n % 64 != 0 and all(n > 2 * l["hist_blocks"] * p["hist_block_rows"] for l in p["levels"])
    js = base_model(2, 1)
    rng = np.random.default_rng(9)
    x = np.empty((n, 2), dtype=np.float32)
    x[:, 0] = rng.integers(0, 10, n)
    x[:, 1] = rng.integers(0, 2, n)
    x[rng.random(n) < 0.01, 0] = np.nan
    cuts = capi.quantile_cuts(x[:5000], NAN)
    y = (margin_of(js, x, NAN) + np.nan_to_num(x[:, 0]) * 0.1 - x[:, 1] + rng.normal(0, 0.1, n)).astype(np.float32)
    w = weights(14, n)
    want, got, b = check(tmp_path, js, x, NAN, y, w, cuts, (x, NAN, y, w), "past the launch caps", max_depth=2, eta=0.5)
    assert len(want["trees"][0]["left"]) == 7 and got["eval_rmse"].tolist() == got["train_rmse"].tolist()
    b.free()


def test_the_form_the_stream_the_order_of_the_rows_and_the_grid_change_no_bit(torch_cuda, tmp_path):
    torch = torch_cuda
    js, x, y, ex, ey, cuts = case(27, 1200, 1300, missing=-999.0, emissing=-999.0)
    w, ew = weights(20, 1200), weights(21, 1300)
    kw = dict(rounds=3, max_depth=5, eta=0.5, patience=2, min_child_weight=0.25)
    want = restate(js, x, -999.0, y, w, cuts, (ex, -999.0, ey, ew), **kw)
    perm, eperm = np.random.default_rng(1).permutation(1200), np.random.default_rng(2).permutation(1300)
    first = None
    for what, p, ep, grid, device in (("plain", None, None, None, "host"), ("rows permuted", perm, eperm, None, "host"),
                                      ("a grid said", None, None, (13, 10, 0), "host"), ("device form on a stream", None, None, None, "device"),
                                      ("device form, permuted, grid said", perm, eperm, (13, 10, 0), "device"),
                                      ("a device held-out matrix in the host form", None, None, None, "mixed")):
        xs, ys, ws = (x, y, w) if p is None else (np.ascontiguousarray(x[p]), y[p].copy(), w[p].copy())
        exs, eys, ews = (ex, ey, ew) if ep is None else (np.ascontiguousarray(ex[ep]), ey[ep].copy(), ew[ep].copy())
        b = capi.Booster(model_buffer=js)
        if device != "host":
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                tx, ty, tw = (torch.from_numpy(a).to("cuda") for a in (xs, ys, ws))
                tex, tey, tew = (torch.from_numpy(a).to("cuda") for a in (exs, eys, ews))
            s.synchronize()
        d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=1200, ncol=27, missing=-999.0) if device == "device" else capi.DMatrix(xs, missing=-999.0)
        ed = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=1300, ncol=27, missing=-999.0) if device != "host" else capi.DMatrix(exs, missing=-999.0)
        if grid is not None:
            d.set_grid(12, 10, 0)
            ed.set_grid(*grid)
        if device == "device":
            got = b.boost_trees_weighted_device(d, ty.data_ptr(), 1200, cuts, weights_ptr=tw.data_ptr(),
                                                eval_set=(ed, tey.data_ptr(), 1300, tew.data_ptr()), stream=s.cuda_stream, **kw)
        else:
            got = b.boost_trees_weighted(d, ys, cuts, weights=ws, eval_set=(ed, eys, ews), **kw)
        same_result(got, want, what)
        same_new_trees(held(b, tmp_path)[0], want["trees"], 3, what)
        image = saved(b, tmp_path)
        first = first or image
        assert image == first, what
        for m in (d, ed):
            m.free()
        b.free()


def test_early_stopping_with_the_best_round_strictly_inside_and_what_follows_a_success(torch_cuda, tmp_path):
    xt, yt, xe, ye, cuts = early_stopping_case()
    wt, we = weights(30, len(yt)), weights(31, len(ye))
    js = G.empty_model(3, base=0.0)
    kw = dict(rounds=20, max_depth=6, eta=0.5, reg_lambda=1.0, patience=3, min_child_weight=1.0)
    want = restate(js, xt, NAN, yt, wt, cuts, (xe, NAN, ye, we), **kw)
    assert 0 < want["best_round"] < want["rounds_run"] < 20
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(xt, missing=NAN)
    ed = capi.DMatrix(xe, missing=NAN)
    got = b.boost_trees_weighted(d, yt, cuts, weights=wt, eval_set=(ed, ye, we), **kw)
    same_result(got, want, "early stopping")
    assert len(got["eval_rmse"]) == want["rounds_run"] + 1
    # the saved model is what the call leaves with rounds = best and no patience
    twin = capi.Booster(model_buffer=js)
    plain = dict(kw, rounds=want["best_round"], patience=0)
    assert twin.boost_trees_weighted(d, yt, cuts, weights=wt, eval_set=(ed, ye, we), **plain)["nodes_added"] == got["nodes_added"]
    assert saved(b, tmp_path) == saved(twin, tmp_path)
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
    for bb in (b, twin):
        bb.free()


# ---- refusals on the GPU ----

def test_refusals_leave_the_model_unchanged_and_a_valid_call_follows(torch_cuda, tmp_path):
    torch = torch_cuda
    js, x, y, ex, ey, cuts = case(3, 1000, 300)
    w, ew = weights(40, 1000), weights(41, 300)
    kw = dict(rounds=2, max_depth=3, patience=1)
    ev = (ex, NAN, ey, ew)
    want = restate(js, x, NAN, y, w, cuts, ev, **kw)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=NAN)
    ed = capi.DMatrix(ex, missing=NAN)
    before = saved(b, tmp_path)

    def valid(what):
        assert saved(b, tmp_path) == before, what
        same_result(b.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ey, ew), **kw), want, what)
        b.load_model_buffer(js)

    for bad in (np.nan, -1.0, 256.0, np.inf):
        wb = w.copy()
        wb[7] = bad
        with pytest.raises(ValueError, match="^weight"):
            restate(js, x, NAN, y, wb, cuts, ev, **kw)
        with pytest.raises(capi.OhxError, match="a weight is not finite") as err:
            b.boost_trees_weighted(d, y, cuts, weights=wb, eval_set=(ed, ey, ew), **kw)
        assert "eval weight" not in str(err.value) and "unchanged" in str(err.value)
        valid(f"a training weight of {bad}")
        eb = ew.copy()
        eb[299] = bad
        with pytest.raises(ValueError, match="^eval weight"):
            restate(js, x, NAN, y, w, cuts, (ex, NAN, ey, eb), **kw)
        with pytest.raises(capi.OhxError, match="eval weight"):
            b.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ey, eb), **kw)
        valid(f"an eval weight of {bad}")
    # all weights zero, on either set
    with pytest.raises(capi.OhxError, match="weights of the training rows sum to 0"):
        b.boost_trees_weighted(d, y, cuts, weights=np.zeros(1000, np.float32), eval_set=(ed, ey, ew), **kw)
    valid("training weights all zero")
    with pytest.raises(capi.OhxError, match="eval weights of the held-out rows sum to 0"):
        b.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ey, np.zeros(300, np.float32)), **kw)
    valid("eval weights all zero")
    # |g * w| >= 256 with |g| < 256
    g0 = margin_of(js, x, NAN) - y
    row = int(np.argmax(np.abs(g0)))
    wb = w.copy()
    wb[row] = np.float32(255.0)
    assert 1.01 < abs(g0[row]) < 256 and abs(np.float32(g0[row]) * wb[row]) >= 256
    with pytest.raises(ValueError, match="^label"):
        restate(js, x, NAN, y, wb, cuts, ev, **kw)
    with pytest.raises(capi.OhxError, match="label") as err:
        b.boost_trees_weighted(d, y, cuts, weights=wb, eval_set=(ed, ey, ew), **kw)
    assert "weight is not finite" not in str(err.value)
    valid("a weighted gradient out of range")
    # a NaN label on a zero-weight row is still a label refused
    yb, wb = y.copy(), w.copy()
    yb[5], wb[5] = np.nan, 0.0
    with pytest.raises(capi.OhxError, match="label") as err:
        b.boost_trees_weighted(d, yb, cuts, weights=wb, eval_set=(ed, ey, ew), **kw)
    assert "eval label" not in str(err.value)
    valid("a NaN label on a zero-weight row")
    # ... and before a bad weight on the same row
    wb[5] = np.nan
    with pytest.raises(capi.OhxError, match="a gradient pred - label"):
        b.boost_trees_weighted(d, yb, cuts, weights=wb, eval_set=(ed, ey, ew), **kw)
    valid("a NaN label and a NaN weight")
    # eval weights without a held-out set
    with pytest.raises(capi.OhxError, match="eval weights are given without a held-out matrix"):
        import ctypes as C
        ptr, vals = b._cuts(cuts)
        r, k = C.c_int32(), C.c_int32()
        capi.check(b.lib, b.lib.OHXBoosterBoostTreesWeighted(b.handle, d.handle, y.ctypes.data, w.ctypes.data, 1000, None, None,
                                                             ew.ctypes.data, 0, ptr.ctypes.data, vals.ctypes.data, 2, 3, 0.3, 1.0,
                                                             0.0, 1.0, 0, None, None, C.byref(r), C.byref(k), None))
    valid("eval weights without a held-out set")
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
            b.boost_trees_weighted_device(dd, ty.data_ptr(), 1000, cuts, weights_ptr=tw.data_ptr(),
                                          eval_set=(de, tey.data_ptr(), 300, tew.data_ptr()),
                                          stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert saved(b, tmp_path) == before, "a captured stream"
    with torch.cuda.stream(s):
        got = b.boost_trees_weighted_device(dd, ty.data_ptr(), 1000, cuts, weights_ptr=tw.data_ptr(),
                                            eval_set=(de, tey.data_ptr(), 300, tew.data_ptr()), stream=s.cuda_stream, **kw)
    same_result(got, want, "after the capture")
    for m in (d, ed, dd, de):
        m.free()
    b.free()
