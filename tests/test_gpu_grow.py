"""Boosting new trees on the GPU (csrc/grow.hip).  Every array of every new tree and nodes_added are compared bit for
bit.

Expected trees never come from the code under test: tests/grow_support.py restates OHXBoosterBoostTrees in numpy from the
text of include/ohxgb.h.  The margin the restatement starts from is a margin predict of a FRESH booster of the same
model (XGBoosterPredict, option_mask = 1: a path held to its own tests).  What the library holds after a call is read
through XGBoosterSaveModel (JSON)."""
import functools
import json

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_support as G
from tests import helpers
from tests import visits_support as V

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def nfeat_of(js):
    return int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])


@functools.lru_cache(maxsize=None)
def base_model(nfeat, ntree=3):
    return V.random_booster(9000 + nfeat, ntree, nfeat, max_depth=4, p_leaf=0.1) if ntree else G.empty_model(nfeat)


def rows(seed, n, nfeat, missing, rate=0.05):
    """Normal columns, every fourth one of few distinct values; `rate` of the values missing, NaN and `missing` both."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (n, nfeat)).astype(np.float32)
    for f in range(1, nfeat, 4):
        x[:, f] = rng.integers(0, 5, n)
    m = rng.random(x.shape)
    x[m < rate] = np.nan
    if not np.isnan(missing):
        x[m < rate / 2] = missing
    return x


def labels(seed, x, margin, scale=1.0):
    """The margin plus a signal in the first columns plus noise: something for a tree to find."""
    rng = np.random.default_rng(seed)
    z = np.nan_to_num(x[:, 0], nan=0.5, posinf=2.0, neginf=-2.0)
    z = np.where(np.abs(z) > 50, 0.5, z)
    s = np.where(z > 0.3, 1.0, -0.5) + (0.3 * np.nan_to_num(x[:, -1], nan=-1.0, posinf=2.0, neginf=-2.0).clip(-3, 3))
    return (margin + scale * (s + rng.normal(0, 0.3, len(x)))).astype(np.float32)


def margin_of(js, x, missing):
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=missing)
    m = b.predict(d, option_mask=1).copy()
    d.free()
    b.free()
    return m


def held(b, tmp_path, name="held.json"):
    path = str(tmp_path / name)
    b.save_model(path)
    image = open(path, "rb").read()
    return G.trees_of(image), image


def same_new_trees(got, want_trees, nold, what=""):
    assert len(got) == nold + len(want_trees), (what, len(got))
    for r, (a, t) in enumerate(zip(got[nold:], want_trees)):
        bad = G.same_tree(a, t)
        assert bad is None, (what, "round", r, bad, a[bad][:8], t[bad][:8])


def check(tmp_path, js, x, missing, y, cuts, what="", grid=None, **kw):
    """One host-form call on a fresh booster against the restatement -> (the restatement, the booster, the matrix)."""
    F = nfeat_of(js)
    pk = {"rounds": kw.get("rounds", 1), "max_depth": kw.get("max_depth", 6), "eta": kw.get("eta", 0.3),
          "lam": kw.get("reg_lambda", 1.0), "gamma": kw.get("gamma", 0.0), "min_child_rows": kw.get("min_child_rows", 1)}
    want = G.boost(margin_of(js, x, missing), x, missing, y, cuts, F, **pk)
    old = G.trees_of(synth.convert_model(js, "json"))
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=missing)
    if grid is not None:
        d.set_grid(*grid)
    n = b.boost_trees(d, y, cuts, **kw)
    got, _ = held(b, tmp_path)
    assert n == want["nodes_added"], (what, n, want["nodes_added"])
    same_new_trees(got, want["trees"], len(old), what)
    for a, o in zip(got, old):
        assert all(np.array_equal(a[k], o[k]) for k in G.ARRAYS), (what, "an old tree changed")
    return want, b, d


def level_sizes(t):
    """Nodes per level of a restated tree."""
    sizes, level = [], [0]
    while level:
        sizes.append(len(level))
        level = [c for n in level if t["left"][n] >= 0 for c in (int(t["left"][n]), int(t["right"][n]))]
    return sizes


def done(b, d):
    d.free()
    b.free()


# ---- new trees against the restatement ----

@pytest.mark.parametrize("nfeat", (1, 3, 27))
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_trees_equal_the_restatement(torch_cuda, tmp_path, n, nfeat):
    """Cuts from the rows themselves, so rows sit on thresholds; NaN and -999 in the rows."""
    missing = -999.0 if (n + nfeat) % 2 else float("nan")
    js = base_model(nfeat)
    x = rows(n * 7 + nfeat, n, nfeat, missing)
    y = labels(n, x, margin_of(js, x, missing))
    cuts = capi.quantile_cuts(x, missing, 64)
    want, b, d = check(tmp_path, js, x, missing, y, cuts, f"{n} rows, {nfeat} features", rounds=2, max_depth=6)
    if n >= 4097:
        assert want["nodes_added"] > 20 and np.isnan(x).any()
    done(b, d)


@pytest.mark.parametrize("max_depth,rounds", [(1, 5), (2, 2), (6, 1), (8, 2)])
def test_depths_and_rounds(torch_cuda, tmp_path, max_depth, rounds):
    js = base_model(3)
    x = rows(max_depth, 4097, 3, -999.0)
    y = labels(rounds, x, margin_of(js, x, -999.0))
    want, b, d = check(tmp_path, js, x, -999.0, y, capi.quantile_cuts(x, -999.0, 255), f"depth {max_depth}",
                       rounds=rounds, max_depth=max_depth, eta=0.5)
    assert all(len(t["left"]) <= 2 ** (max_depth + 1) - 1 for t in want["trees"])
    if max_depth == 8:
        assert max(max(level_sizes(t)[:8]) for t in want["trees"]) > 53, "a level of more than 53 open nodes"
    done(b, d)


def test_128_features_at_depth_8_take_several_node_and_feature_groups(torch_cuda, tmp_path):
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, F = 4097, 128
    p = synth.grow_plan(n, F, 0, 8, cus)
    assert p["levels"][7]["node_groups"] >= 2 and p["levels"][7]["feat_groups"] >= 2 and p["levels"][0]["feat_groups"] >= 2
    js = base_model(F, 2)
    rng = np.random.default_rng(128)
    x = rng.normal(0, 1, (n, F)).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    y = (margin_of(js, x, float("nan")) + np.nan_to_num(x[:, 5] * x[:, 100]) + np.nan_to_num(x[:, 127])).astype(np.float32)
    want, b, d = check(tmp_path, js, x, float("nan"), y, capi.quantile_cuts(x, float("nan"), 8), "128 features",
                       max_depth=8, eta=0.3, min_child_rows=4)
    assert max(level_sizes(want["trees"][0])[:8]) > 53, "more open nodes at a level than one block holds"
    done(b, d)


def test_zero_one_and_254_cuts_a_duplicated_column_and_a_column_in_one_bin(torch_cuda, tmp_path):
    n = 4097
    rng = np.random.default_rng(254)
    x = np.zeros((n, 6), dtype=np.float32)
    x[:, 0] = 7.0                                   # constant: no cuts
    x[:, 1] = rng.integers(0, 2, n)                 # one cut: every add of a block lands on two addresses
    x[:, 2] = rng.normal(0, 1, n)                   # 254 cuts
    x[:, 3] = x[:, 2]                               # a duplicated column: the lower feature wins every tie
    x[:, 4] = rng.normal(0, 1, n) + 100.0           # cuts given below, every row above them: one bin
    x[:, 5] = rng.normal(0, 1, n)
    ptr, vals = capi.quantile_cuts(x, float("nan"), 255)
    counts = np.diff(ptr.astype(np.int64))
    assert counts[0] == 0 and counts[1] == 1 and counts[2] == 254 and counts[3] == 254
    # feature 4: three cuts far below its rows
    a, e = int(ptr[4]), int(ptr[5])
    vals = np.concatenate([vals[:a], np.array([-3, -2, -1], np.float32), vals[e:]])
    ptr = ptr.copy()
    ptr[5:] = ptr[5:] - (e - a) + 3
    cuts = (ptr, vals)
    js = base_model(6)
    y = (margin_of(js, x, float("nan")) + np.where(x[:, 2] > 0.1, 1.0, -1.0) + 0.5 * x[:, 1] + 0.2 * x[:, 5]).astype(np.float32)
    want, b, d = check(tmp_path, js, x, float("nan"), y, cuts, "cut counts", rounds=2, max_depth=5)
    used = np.concatenate([t["feature"][t["left"] >= 0] for t in want["trees"]])
    assert 2 in used and 3 not in used and 0 not in used and 4 not in used
    done(b, d)


def test_inf_in_a_device_matrix_and_fewer_columns_than_features(torch_cuda, tmp_path):
    torch = torch_cuda
    n, F = 1000, 5
    js = base_model(F)
    x = rows(11, n, 3, float("nan"))                # three columns of five features
    x[::50, 0] = np.inf
    x[7::50, 2] = -np.inf
    cuts3 = capi.quantile_cuts(x, float("nan"), 32)
    cuts = (np.concatenate([cuts3[0], cuts3[0][-1:], cuts3[0][-1:]]), cuts3[1])
    tx = torch.from_numpy(x).cuda()
    d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=n, ncol=3, missing=float("nan"))
    fresh = capi.Booster(model_buffer=js)
    tm = torch.zeros(n, dtype=torch.float32, device="cuda")
    fresh.predict_device(d, tm.data_ptr(), option_mask=1)
    torch.cuda.synchronize()
    margin = tm.cpu().numpy()
    fresh.free()
    y = labels(5, x, margin)
    ty = torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    want = G.boost(margin, x, float("nan"), y, cuts, F, rounds=2, max_depth=4)
    b = capi.Booster(model_buffer=js)
    assert b.boost_trees_device(d, ty.data_ptr(), n, cuts, rounds=2, max_depth=4) == want["nodes_added"]
    same_new_trees(held(b, tmp_path)[0], want["trees"], 3, "inf, three columns of five")
    # the booster's sticky inf flag is as it was: a host matrix predicts
    clean = capi.DMatrix(np.zeros((4, 3), np.float32), missing=float("nan"))
    assert len(b.predict(clean, option_mask=1)) == 4
    done(b, d)
    clean.free()


def test_labels_that_make_every_gradient_zero_leave_the_root_a_leaf(torch_cuda, tmp_path):
    js = base_model(3)
    x = rows(2, 300, 3, float("nan"))
    m = margin_of(js, x, float("nan"))
    want, b, d = check(tmp_path, js, x, float("nan"), m.copy(), capi.quantile_cuts(x, float("nan")), "zero gradients", rounds=2)
    for t in want["trees"]:
        assert len(t["left"]) == 1 and t["value"][0] == 0.0 and t["sum_hess"][0] == 300.0
    assert np.signbit(want["trees"][0]["value"][0]), "-(0) / (H + lambda) is -0.0"
    done(b, d)


def test_min_child_rows_larger_than_half_the_rows(torch_cuda, tmp_path):
    js = base_model(3)
    x = rows(3, 200, 3, float("nan"))
    y = labels(3, x, margin_of(js, x, float("nan")))
    cuts = capi.quantile_cuts(x, float("nan"))
    want, b, d = check(tmp_path, js, x, float("nan"), y, cuts, "no child is large enough", min_child_rows=101)
    assert len(want["trees"][0]["left"]) == 1 and want["trees"][0]["value"][0] != 0.0
    done(b, d)
    want, b, d = check(tmp_path, js, x, float("nan"), y, cuts, "one split at most per path", min_child_rows=60, max_depth=4)
    assert len(want["trees"][0]["left"]) == 3
    done(b, d)
    want, b, d = check(tmp_path, js, x, float("nan"), y, cuts, "gamma above every gain", gamma=1e6)
    assert len(want["trees"][0]["left"]) == 1
    done(b, d)


def test_more_rows_than_two_trips_of_each_kernels_loop(torch_cuda, tmp_path):
    """A block strides over its rows.  The trips come from the plan the library exports.  Feature 1 has one cut, so every
    add of a block lands on two LDS addresses."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = synth.grow_plan(1 << 30, 2, 10, 2, cus)
    trip = max(full["row_blocks"] * full["block_rows"], max(l["hist_blocks"] for l in full["levels"]) * full["hist_block_rows"])
    n = 2 * trip + 77
    p = synth.grow_plan(n, 2, 10, 2, cus)
    assert n % 64 != 0 and n > 2 * p["row_blocks"] * p["block_rows"]
    assert all(n > 2 * l["hist_blocks"] * p["hist_block_rows"] for l in p["levels"])
    js = base_model(2, 1)
    rng = np.random.default_rng(9)
    x = np.empty((n, 2), dtype=np.float32)
    x[:, 0] = rng.integers(0, 10, n)
    x[:, 1] = rng.integers(0, 2, n)
    x[rng.random(n) < 0.01, 0] = np.nan
    cuts = capi.quantile_cuts(x[:5000], float("nan"))
    assert np.diff(cuts[0].astype(np.int64)).tolist() == [9, 1]
    y = (margin_of(js, x, float("nan")) + np.nan_to_num(x[:, 0]) * 0.1 - x[:, 1] + rng.normal(0, 0.1, n)).astype(np.float32)
    want, b, d = check(tmp_path, js, x, float("nan"), y, cuts, "past the launch caps", max_depth=2, eta=0.5)
    assert len(want["trees"][0]["left"]) == 7
    done(b, d)


# ---- independence ----

def test_the_order_of_the_rows_the_form_and_the_grid_change_no_bit(torch_cuda, tmp_path):
    torch = torch_cuda
    js = base_model(27)
    n = 1200
    x = rows(12, n, 27, -999.0)
    y = labels(12, x, margin_of(js, x, -999.0))
    cuts = capi.quantile_cuts(x, -999.0, 32)
    want = G.boost(margin_of(js, x, -999.0), x, -999.0, y, cuts, 27, rounds=2, max_depth=5)
    perm = np.random.default_rng(1).permutation(n)
    xp, yp = np.ascontiguousarray(x[perm]), np.ascontiguousarray(y[perm])
    for what, rws, lab, grid, device in (("plain", x, y, None, False), ("permuted", xp, yp, None, False),
                                         ("grid said", x, y, (12, 10, 0), False), ("device form", x, y, None, True),
                                         ("device form, grid said, permuted", xp, yp, (12, 10, 0), True)):
        b = capi.Booster(model_buffer=js)
        if device:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                tx = torch.from_numpy(rws).to("cuda")
                ty = torch.from_numpy(lab).to("cuda")
            s.synchronize()
            d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=n, ncol=27, missing=-999.0)
        else:
            d = capi.DMatrix(rws, missing=-999.0)
        if grid is not None:
            d.set_grid(*grid)
        if device:
            got_n = b.boost_trees_device(d, ty.data_ptr(), n, cuts, rounds=2, max_depth=5, stream=s.cuda_stream)
        else:
            got_n = b.boost_trees(d, lab, cuts, rounds=2, max_depth=5)
        assert got_n == want["nodes_added"], what
        same_new_trees(held(b, tmp_path)[0], want["trees"], 3, what)
        done(b, d)


# ---- where the call starts from ----

def test_from_a_model_without_trees(torch_cuda, tmp_path):
    js = G.empty_model(3, base=0.25)
    x = rows(4, 500, 3, float("nan"))
    y = labels(4, x, np.full(500, 0.25, np.float32))
    assert np.array_equal(margin_of(js, x, float("nan")), np.full(500, 0.25, np.float32))
    want, b, d = check(tmp_path, js, x, float("nan"), y, capi.quantile_cuts(x, float("nan")), "0 trees", rounds=3, max_depth=3)
    assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want["pred"]))
    done(b, d)


def test_from_every_kind_of_tree(torch_cuda, tmp_path):
    js, trees = S.make_booster(8010, 10)
    assert {k for k in S.SMALL_PLANS[10]} == set(S.KINDS)
    x = S.rows_for(77, trees, 2000, -999.0)
    y = labels(8, x, margin_of(js, x, -999.0))
    want, b, d = check(tmp_path, js, x, -999.0, y, capi.quantile_cuts(x, -999.0, 64), "every kind", rounds=2, max_depth=4)
    assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want["pred"]))
    done(b, d)


# ---- after a success ----

def test_after_a_success_everything_follows_the_longer_forest(torch_cuda, tmp_path):
    js0, trees = S.contribs_booster(8105, 10)
    n = 4097
    x = S.rows_for(31, trees, n, -999.0)
    y = labels(9, x, margin_of(js0, x, -999.0))
    cuts = capi.quantile_cuts(x, -999.0, 64)
    pk = dict(rounds=3, max_depth=5, eta=0.5)
    b = capi.Booster(model_buffer=js0)
    d = capi.DMatrix(x, missing=-999.0)
    dx = capi.DMatrix(x[:96], missing=-999.0)
    # the refit state, the device forests, the contributions state and the visit counters exist before the call: the
    # user's own sequence - refit the frozen structure first, then boost on what remains
    b.refit_leaves(d, y, eta=0.5)
    old_json, js = held(b, tmp_path, "old.json")
    margin = b.predict(d, option_mask=1).copy()
    before = margin
    assert np.array_equal(helpers.bits(margin), helpers.bits(margin_of(js, x, -999.0)))
    b.predict_contribs(dx)
    b.predict_contribs(dx, approximate=True)
    b.count_visits(d)
    assert b.visit_counts()[1] == n
    want = G.boost(margin, x, -999.0, y, cuts, 27, **pk)
    other = capi.Booster(model_buffer=G.with_trees(js, want["trees"]))
    assert b.boost_trees(d, y, cuts, **pk) == want["nodes_added"]
    got, image = held(b, tmp_path)
    same_new_trees(got, want["trees"], 10, "after state was built")
    for a, o in zip(got, old_json):
        assert all(np.array_equal(a[k], o[k]) for k in G.ARRAYS), "an old tree changed"
    # margins: the restatement's running pred, by every kernel, and a booster loaded from the restatement's JSON
    for kernel, split in (("auto", "auto"), ("wide", "auto"), ("ring", "off")):
        for bb in (b, other):
            bb.set_param("ohx_kernel", kernel)
            bb.set_param("ohx_tree_split", split)
        got_m, ref_m = b.predict(d, option_mask=1), other.predict(d, option_mask=1)
        assert np.array_equal(helpers.bits(got_m), helpers.bits(ref_m)), kernel
        assert np.array_equal(helpers.bits(got_m), helpers.bits(want["pred"])), kernel
    assert np.array_equal(b.predict(d, option_mask=16), other.predict(d, option_mask=16))
    # contributions run at once and sum to the margin within the bound of tests/test_gpu_contribs.py
    m = b.predict(dx, option_mask=1).astype(np.float64)
    for approximate in (False, True):
        phi = b.predict_contribs(dx, approximate=approximate).astype(np.float64)
        assert np.all(np.abs(phi.sum(axis=1) - m) <= 1e-5 * (1.0 + np.abs(phi).sum(axis=1))), approximate
    # the visit counters went with the old leaf numbering; a count over the training rows gives every new node its cover
    counts, seen = b.visit_counts()
    assert seen == 0 and len(counts) == 13 and all(int(c.sum()) == 0 for c in counts)
    b.count_visits(d)
    counts, seen = b.visit_counts()
    assert seen == n
    for t, tree in zip(counts[10:], want["trees"]):
        assert np.array_equal(helpers.bits(t.astype(np.float32)), helpers.bits(tree["sum_hess"]))
    # the three file formats reload to the same arrays
    for ext in ("json", "ubj", "bin"):
        path = str(tmp_path / f"grown.{ext}")
        b.save_model(path)
        again = capi.Booster(model_file=path)
        back, _ = held(again, tmp_path, f"back_{ext}.json")
        same_new_trees(back, want["trees"], 10, ext)
        for a, o in zip(back, old_json):
            assert all(np.array_equal(a[k], o[k]) for k in G.ARRAYS), ext
        assert np.array_equal(helpers.bits(again.predict(d, option_mask=1)), helpers.bits(want["pred"])), ext
        again.free()
    # a second call continues from the first
    more = G.boost(want["pred"], x, -999.0, y, cuts, 27, rounds=2, max_depth=3, eta=0.5)
    assert b.boost_trees(d, y, cuts, rounds=2, max_depth=3, eta=0.5) == more["nodes_added"]
    same_new_trees(held(b, tmp_path)[0], want["trees"] + more["trees"], 10, "a second call")
    # training RMSE falls, as the restatement itself shows on this input
    rmse = lambda p: float(np.sqrt(np.mean((p.astype(np.float64) - y) ** 2)))
    assert rmse(want["pred"]) < rmse(margin) and rmse(more["pred"]) < rmse(want["pred"])
    assert rmse(b.predict(d, option_mask=1)) < rmse(before)
    dx.free()
    done(b, d)
    other.free()


# ---- all or nothing ----

def test_refusals_leave_margins_and_saved_bytes_unchanged_and_a_valid_call_follows(torch_cuda, tmp_path):
    torch = torch_cuda
    js = base_model(3)
    n = 1000
    x = rows(6, n, 3, -999.0)
    margin = margin_of(js, x, -999.0)
    y = labels(6, x, margin)
    cuts = capi.quantile_cuts(x, -999.0, 32)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=-999.0)
    path = str(tmp_path / "before.json")
    b.save_model(path)
    saved = open(path, "rb").read()

    def untouched(what):
        assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(margin)), what
        b.save_model(path)
        assert open(path, "rb").read() == saved, what

    def valid(what):
        """A valid call on a copy of the state: the booster stays usable (the model is put back afterwards)."""
        want = G.boost(margin, x, -999.0, y, cuts, 3, rounds=1, max_depth=3)
        assert b.boost_trees(d, y, cuts, rounds=1, max_depth=3) == want["nodes_added"], what
        same_new_trees(held(b, tmp_path)[0], want["trees"], 3, what)
        b.load_model_buffer(js)

    yb = y.copy()
    yb[777] = np.nan
    with pytest.raises(ValueError):
        G.boost(margin, x, -999.0, yb, cuts, 3)
    with pytest.raises(capi.OhxError, match="label") as e:
        b.boost_trees(d, yb, cuts)
    assert "unchanged" in str(e.value)
    untouched("a NaN label")
    valid("after a NaN label")
    # |g| >= 256 first reached at round 2: g = 200 everywhere, lambda = 0, eta = 3: round 1 is a root leaf of -600
    yl = (margin - np.float32(200.0)).astype(np.float32)
    with pytest.raises(ValueError, match="round 1"):
        G.boost(margin, x, -999.0, yl, cuts, 3, rounds=3, eta=3.0, lam=0.0, gamma=1e9)
    with pytest.raises(capi.OhxError, match="label"):
        b.boost_trees(d, yl, cuts, rounds=3, eta=3.0, reg_lambda=0.0, gamma=1e9)
    untouched("a gradient out of range at round 2")
    valid("after a late refusal")
    for nl in (n - 1, n + 1):
        with pytest.raises(capi.OhxError, match=f"{nl} labels for {n} rows"):
            b.boost_trees(d, np.zeros(nl, np.float32), cuts)
    wide = capi.DMatrix(np.zeros((4, 4), dtype=np.float32), missing=-999.0)
    with pytest.raises(capi.OhxError, match="Number of columns"):
        b.boost_trees(wide, np.zeros(4, np.float32), cuts)
    wide.free()
    untouched("mismatched counts")
    valid("after mismatched counts")
    # a stream that is being captured
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    dd = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=n, ncol=3, missing=-999.0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="stream capture"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.boost_trees_device(dd, ty.data_ptr(), n, cuts, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    untouched("a captured stream")
    want = G.boost(margin, x, -999.0, y, cuts, 3, rounds=1, max_depth=3)
    with torch.cuda.stream(s):
        assert b.boost_trees_device(dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=3, stream=s.cuda_stream) == want["nodes_added"]
    same_new_trees(held(b, tmp_path)[0], want["trees"], 3, "after the capture")
    dd.free()
    done(b, d)


def test_no_rows_and_too_many_rows(torch_cuda, tmp_path):
    """Matrices that borrow device memory with a made-up row count: refused before a row or a label is read."""
    torch = torch_cuda
    tx = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    ty = torch.zeros(64, dtype=torch.float32, device="cuda")
    b = capi.Booster(model_buffer=base_model(3))
    cuts = (np.arange(4, dtype=np.uint64), np.zeros(3, np.float32))
    empty = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=0, ncol=3, missing=-999.0)
    with pytest.raises(capi.OhxError, match="the matrix has no rows"):
        b.boost_trees_device(empty, ty.data_ptr(), 0, cuts)
    many = (1 << 31) + 1
    over = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=many, ncol=3, missing=-999.0)
    with pytest.raises(capi.OhxError, match="at most 2\\^31 rows"):
        b.boost_trees_device(over, ty.data_ptr(), many, cuts)
    assert len(held(b, tmp_path)[0]) == 3
    for m in (empty, over):
        m.free()
    b.free()
