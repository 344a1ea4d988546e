""""ohx_colsample_bylevel" and "ohx_colsample_bynode" on the GPU (csrc/grow_colsample.hip, through XGBoosterSetParam and
colsample_bylevel= / colsample_bynode= of the Python binding).  Every array of every new tree, nodes_added, rounds_run and
best_round are compared as integers or bit for bit, both metric arrays with ==, and models byte for byte in all three
formats.

The expected values are the restatement's (tests/grow_colsample_support.py, written from the header) and, where the header
states an equality (C1, C3, rows permuted), another call on a twin booster.  The model of a case has no tree unless the case
says so, so the margin a restatement starts from is the model's base.  What a case is meant to reach is asserted from the
restatement before the GPU is asked: above all a node whose best candidate over the tree's features lies outside the node's
own (grow_colsample_support.narrowed) - without one the case would pass on the code path of a call without the two parameters.  A row
alone and a feature alone can have no such node (nothing splits; nothing is drawn): those two cases say so.  C2 is computed
from the trees the library returns and the restated draws alone, for every case.  Every tree here grows at one point of
eta, lambda, min_child_weight and gamma (call_kw), and C2 asks only that a split's feature is the node's own: gamma > 0,
min_child_weight > 0 and lambda 0 under the fractions, and whether a split is the best of the node's own columns, asked
of the library's tree by the exact audit, are tests/test_gpu_grow_audit.py's."""
import ctypes as C

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_colsample_support as K
from tests import grow_deep_support as D
from tests import grow_mono_support as M
from tests import grow_objective_support as O
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests.test_gpu_grow import held, same_new_trees
from tests.test_gpu_grow_eval import same_result, saved
from tests.test_gpu_grow_objective import NAN, booster, call, done, same_arrays

pytestmark = pytest.mark.gpu

F32 = np.float32
NAMES = ("ohx_colsample_bylevel", "ohx_colsample_bynode")
DRAW_SEED = 29


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def case(kind, n, nfeat, bins, depth, bylevel, bynode, seed=290, rounds=2, subsample=1.0, colsample=1.0, objective="squarederror",
         alpha=0.0, m=0.0, metric="rmse", constraints=(), held_out=0, patience=0, device=False, weighted=True):
    return dict(kind=kind, n=n, nfeat=nfeat, bins=bins, depth=depth, bylevel=bylevel, bynode=bynode, seed=seed, rounds=rounds,
                subsample=subsample, colsample=colsample, objective=objective, alpha=alpha, m=m, metric=metric,
                constraints=tuple(constraints), held_out=held_out, patience=patience, device=device, weighted=weighted)


def restate(c):
    """-> (x, y, w, cuts, ev, the restatement's dict) of a case, computed once."""
    return K.restated(c["bylevel"], c["bynode"], c["constraints"], c["objective"], 1.0, c["alpha"], c["m"], c["metric"], c["n"], c["seed"],
                      c["depth"], bins=c["bins"], nfeat=c["nfeat"], rounds=c["rounds"], held_out=c["held_out"], patience=c["patience"],
                      subsample=c["subsample"], colsample=c["colsample"], draw_seed=DRAW_SEED, weighted=c["weighted"])


def params_of(c):
    return (("ohx_colsample_bylevel", repr(float(c["bylevel"]))), ("ohx_colsample_bynode", repr(float(c["bynode"]))),
            ("ohx_monotone_constraints", "(" + ",".join(str(v) for v in c["constraints"]) + ")"), ("ohx_objective", c["objective"]),
            ("ohx_huber_slope", "1.0"), ("ohx_reg_alpha", repr(float(c["alpha"]))), ("ohx_max_delta_step", repr(float(c["m"]))),
            ("ohx_eval_metric", c["metric"]))


def call_kw(c):
    return dict(eta=0.125, reg_lambda=1.0, min_child_weight=0.0, max_depth=c["depth"], rounds=c["rounds"], subsample=c["subsample"],
                colsample_bytree=c["colsample"], seed=DRAW_SEED, patience=c["patience"])


def depths_of(t):
    """The depth of every node of the tree arrays `t`, the root's being 0 (children follow their parent in the arrays)."""
    d = np.zeros(len(t["left"]), dtype=np.int64)
    for i in range(len(d)):
        if t["left"][i] >= 0:
            d[t["left"][i]] = d[t["right"][i]] = d[i] + 1
    return d


def check_c2(trees, nfeat, bylevel, bynode, colsample, tree0=0):
    """C2 from the returned trees and the restated draws alone -> the split nodes looked at."""
    seen = 0
    for r, t in enumerate(trees):
        i = tree0 + r
        tree_list = P.features(DRAW_SEED, i, nfeat, colsample)
        depth = depths_of(t)
        by_level = {}
        for p in np.flatnonzero(np.asarray(t["left"]) >= 0):
            d, f = int(depth[p]), int(t["feature"][p])
            lvl = by_level.setdefault(d, K.level_features(DRAW_SEED, i, d, tree_list, bylevel))
            assert f in lvl, ("C2: the level's list", i, int(p), d, f, lvl)
            assert f in K.node_features(DRAW_SEED, i, int(p), lvl, bynode), ("C2: the node's list", i, int(p), d, f)
            if len(lvl) == 1:
                assert f == lvl[0]
            seen += 1
    return seen


def check(torch, tmp_path, c, want, x, y, w, cuts, ev, what):
    """One call on a fresh booster against the restatement: the parameters by XGBoosterSetParam in the device form (on a
    stream of its own), by the binding's keyword arguments in the host form."""
    kind, kw = c["kind"], call_kw(c)
    if c["device"]:
        b = booster(params_of(c), nfeat=c["nfeat"])
        got, mats = call(torch, b, kind, x, y, w, cuts, ev, device=True, **kw)
    else:
        b = booster((), nfeat=c["nfeat"])
        got, mats = call(torch, b, kind, x, y, w, cuts, ev, objective=c["objective"], huber_slope=1.0, reg_alpha=c["alpha"],
                         max_delta_step=c["m"], eval_metric=c["metric"], monotone_constraints=c["constraints"],
                         colsample_bylevel=c["bylevel"], colsample_bynode=c["bynode"], **kw)
    same_result(got, want, what)
    trees = held(b, tmp_path)[0]
    same_new_trees(trees, want["trees"], 0, what)
    check_c2(trees, c["nfeat"], c["bylevel"], c["bynode"], c["colsample"])
    image = saved(b, tmp_path)
    done(b, mats)
    return got, image, trees


# ---- 1. rows, features and depths at their edges ----

# rows: one alone, a wave less one, a wave, a wave and one, more than a block; features 1, 3, 27 and 128 - at 128 and depth 8
# with 64 and 38 columns a level (a last feature group that is not full) and with 96 (a rank over two keys a lane); depths
# 1, 2, 6 and 8 on the LDS path, 9 and 12 on the deep one; each fraction alone, and both
SHAPES = (case("sampled", 1, 1, 8, 1, 0.5, 0.5, weighted=False),
          case("sampled", 63, 3, 64, 2, 0.34, 1.0, seed=291),
          case("sampled", 64, 27, 16, 6, 1.0, 0.5, seed=292),
          case("sampled", 65, 128, 8, 8, 0.5, 0.5, seed=293),
          case("sampled", 4097, 128, 4, 8, 0.3, 1.0, seed=294, rounds=1),
          case("sampled", 4097, 128, 4, 8, 0.75, 0.5, seed=295, rounds=1),
          case("sampled", 4097, 1, 64, 6, 0.99, 0.99, seed=296),
          case("deep_sampled", 4097, 3, 16, 9, 0.67, 0.5, seed=297),
          case("deep_sampled", 4097, 27, 4, 12, 0.5, 0.5, seed=298, rounds=1))


def reaches(c, want):
    """What the case is there for, from the restatement alone."""
    if c["n"] == 1:
        assert want["nodes_added"] == c["rounds"], "a row alone: a root a round, and no node to narrow"
    elif c["nfeat"] == 1:
        assert want["draws"] is None and want["nodes_added"] > 2 * c["rounds"], "a feature alone: nothing is drawn"
    else:
        assert K.narrowed(want["draws"]) >= 1, "a node whose best candidate over the tree's features is not its own"
    if c["depth"] > 8:
        assert any(D.depth_of(t) > 8 and D.levels(t)[8][1] > 0 for t in want["all_trees"]), "level 8 splits: the hand-over"


@pytest.mark.parametrize("c", SHAPES, ids=lambda c: f"{c['n']}x{c['nfeat']}-d{c['depth']}-{c['bylevel']}-{c['bynode']}")
def test_shapes_against_the_restatement(torch_cuda, tmp_path, c):
    x, y, w, cuts, ev, want = restate(c)
    reaches(c, want)
    check(torch_cuda, tmp_path, c, want, x, y, w, cuts, ev, str(c))


# ---- 2. everything the fractions compose with ----

MONO = (1, 0, 0, -1, 0, 0, 0, 0)
OPTIONS = (
    # bylevel alone without a bag or a tree's list, one round, the host form
    case("sampled", 1300, 8, 32, 6, 0.5, 1.0, rounds=1, held_out=400),
    # bynode alone, pseudo-Huber, the device form on its own stream
    case("sampled", 1300, 8, 32, 6, 1.0, 0.5, objective="pseudohuber", held_out=400, device=True),
    # both on top of a bag and a tree's list, regularised, mae with patience, five rounds
    case("sampled", 1300, 8, 32, 6, 0.5, 0.5, rounds=5, subsample=0.5, colsample=0.5, alpha=0.5, m=0.5, metric="mae", held_out=400, patience=2),
    # an active monotone list
    case("sampled", 1300, 8, 32, 6, 0.5, 0.5, constraints=MONO, held_out=400, device=True),
    # the deep path: both on top of a bag and a list, pseudo-Huber with its own metric and alpha
    case("deep_sampled", 8193, 8, 32, 10, 0.5, 0.5, subsample=0.5, colsample=0.5, objective="pseudohuber", alpha=0.5, metric="pseudohuber",
         held_out=400),
    # the deep path under constraints and a step, the device form
    case("deep_sampled", 4097, 8, 32, 10, 0.75, 0.67, constraints=MONO, m=0.5, held_out=400, device=True),
)


@pytest.mark.parametrize("c", OPTIONS, ids=lambda c: "-".join(str(c[k]) for k in ("kind", "objective", "alpha", "m", "metric", "bylevel", "bynode",
                                                                                  "subsample", "rounds")) + ("-mono" if c["constraints"] else ""))
def test_what_the_fractions_compose_with(torch_cuda, tmp_path, c):
    x, y, w, cuts, ev, want = restate(c)
    reaches(c, want)
    assert (w == 0).any() and np.isnan(x).any(), "rows of weight 0 and missing values"
    if c["patience"]:       # (the call waits once a round for the held-out sum)
        assert want["rounds_run"] == c["rounds"] and want["best_round"] == c["rounds"] and want["eval_rmse"] is not None
    _, _, trees = check(torch_cuda, tmp_path, c, want, x, y, w, cuts, ev, str(c))
    if c["constraints"]:        # the monotonicity sweep still holds: each new tree, walked on the host from the returned arrays
        for f, cf in enumerate(c["constraints"]):
            if cf:
                rows = M.sweep_rows(x[:32], f, M.sweep_values(cuts, f))
                assert all(M.violations(M.tree_values(t, rows), cf) == 0 for t in trees), ("monotone in feature", f)
        assert any(np.any(np.isin(t["feature"][t["left"] >= 0], (0, 3))) for t in trees), "a constrained feature is split on"


# ---- 3. a forest to start from, and a second call on one booster ----

def test_a_second_call_on_one_booster_draws_for_its_own_trees(torch_cuda, tmp_path):
    """T0 moves the draw: the second call's trees are trees 2 and 3 of the draws, from the margin the first call left; NaN
    and -999 in the columns."""
    n, nfeat = 1300, 8
    x, y, w, _, ev = O.inputs(n, 299, nfeat, 32, 400)
    x = x.copy()
    x[::7, 0] = -999.0
    x[3::11, 5] = -999.0
    cuts = G.quantile_cuts(x, NAN, 32)
    kw = dict(rounds=2, max_depth=6, eta=0.125, lam=1.0, min_child_weight=0.0, seed=DRAW_SEED)
    first = K.boost(0.5, 0.5, (), "squarederror", 1.0, 0.0, 0.0, "rmse", np.full(n, O.BASE, F32), x, NAN, y, w, cuts, nfeat, eval_set=ev,
                    eval_pred=np.full(400, O.BASE, F32), **kw)
    second = K.boost(0.5, 0.5, (), "squarederror", 1.0, 0.0, 0.0, "rmse", first["pred"], x, NAN, y, w, cuts, nfeat, eval_set=ev,
                     eval_pred=first["eval_pred"], tree0=2, **kw)
    again = K.boost(0.5, 0.5, (), "squarederror", 1.0, 0.0, 0.0, "rmse", first["pred"], x, NAN, y, w, cuts, nfeat, eval_set=ev,
                    eval_pred=first["eval_pred"], tree0=0, **kw)
    assert K.narrowed(first["draws"]) >= 1 and K.narrowed(second["draws"]) >= 1
    assert not M.same_trees(second["trees"], again["trees"]), "with T0 = 0 the second call would grow other trees"
    b = booster((), nfeat=nfeat)
    d, ed = capi.DMatrix(x, missing=NAN), capi.DMatrix(ev[0], missing=NAN)
    bkw = dict(rounds=2, max_depth=6, eta=0.125, reg_lambda=1.0, min_child_weight=0.0, seed=DRAW_SEED, eval_set=(ed, ev[2], ev[3]))
    got = b.boost_trees_sampled(d, y, cuts, weights=w, colsample_bylevel=0.5, colsample_bynode=0.5, **bkw)
    same_result(got, first, "the first call")
    got = b.boost_trees_sampled(d, y, cuts, weights=w, **bkw)        # (None leaves the handle's setting)
    same_result(got, second, "the second call")
    trees = held(b, tmp_path)[0]
    same_new_trees(trees, first["trees"] + second["trees"], 0, "both calls")
    assert check_c2(trees[2:], nfeat, 0.5, 0.5, 1.0, tree0=2) > 10
    done(b, [d, ed])


# ---- 4. C1: fractions that take no feature away ----

@pytest.mark.parametrize("kind,nfeat,fractions", (("sampled", 8, (1.0, 1.0)), ("deep_sampled", 8, (1.0, 1.0)), ("sampled", 1, (0.99, 0.99)),
                                                  ("deep_sampled", 1, (0.99, 0.99)), ("sampled", 2, (0.99, 1.0))))
def test_c1_the_call_is_the_one_it_is_today(torch_cuda, tmp_path, kind, nfeat, fractions):
    """(0.99 of 2 features is 1: the last case is the counter-example, a level that does lose a feature)"""
    x, y, w, cuts, ev = O.inputs(4097, 300, nfeat, 32, 400)
    kw = dict(eta=0.125, reg_lambda=1.0, min_child_weight=0.0, max_depth=10 if "deep" in kind else 6, rounds=2, subsample=0.5,
              colsample_bytree=0.5, seed=DRAW_SEED)
    results = []
    for params in ((), tuple(zip(NAMES, (repr(v) for v in fractions)))):
        b = booster(params, nfeat=nfeat)
        got, mats = call(torch_cuda, b, kind, x, y, w, cuts, ev, **kw)
        results.append((got, saved(b, tmp_path)))
        done(b, mats)
    assert results[0][0]["nodes_added"] > 20
    if K.draws_nothing(P.num_selected(nfeat, 0.5), *fractions):
        same_arrays(results[1][0], results[0][0], kind)
        assert results[1][1] == results[0][1], "bytes in three formats"
    else:
        assert results[1][1] != results[0][1], "a level of one feature of two"


# ---- 5. C2 with one feature a level ----

def test_c2_with_one_feature_a_level_every_split_of_a_level_is_on_it(torch_cuda, tmp_path):
    nfeat = 8
    x, y, w, cuts, _ = O.inputs(4097, 301, nfeat, 32, 0)
    b = booster((), nfeat=nfeat)
    got, mats = call(torch_cuda, b, "deep_sampled", x, y, w, cuts, None, eta=0.125, reg_lambda=1.0, min_child_weight=0.0, max_depth=10,
                     rounds=2, seed=DRAW_SEED, colsample_bylevel=2.0 ** -20, colsample_bynode=0.5)
    trees = held(b, tmp_path)[0]
    assert check_c2(trees, nfeat, 2.0 ** -20, 0.5, 1.0) > 50
    for t in trees:
        depth, split = depths_of(t), np.asarray(t["left"]) >= 0
        per_level = [set(np.asarray(t["feature"])[split & (depth == d)].tolist()) for d in range(10)]
        assert all(len(s) <= 1 for s in per_level) and len(set().union(*per_level)) > 1, per_level
    done(b, mats)


# ---- 6. C3, rows permuted, the grid ----

def test_c3_and_rows_permuted(torch_cuda, tmp_path):
    nfeat, n = 8, 1300
    x, y, w, cuts, ev = O.inputs(n, 302, nfeat, 32, 400)
    kw = dict(eta=0.125, reg_lambda=1.0, min_child_weight=0.0, max_depth=8, rounds=2, colsample_bytree=0.75, seed=DRAW_SEED,
              colsample_bylevel=0.5, colsample_bynode=0.67)
    images, results = [], []
    order = np.random.default_rng(303).permutation(n)
    for kind, rows, labels, weights, grid in (("sampled", x, y, w, False), ("deep_sampled", x, y, w, False),
                                              ("sampled", np.ascontiguousarray(x[order]), y[order], w[order], True)):
        b = booster((), nfeat=nfeat)
        got, mats = call(torch_cuda, b, kind, rows, labels, weights, cuts, ev, grid=grid, **kw)
        results.append(got)
        images.append(saved(b, tmp_path))
        done(b, mats)
    assert results[0]["nodes_added"] > 40
    same_arrays(results[1], results[0], "C3")
    assert images[1] == images[0], "C3: DeepSampled at max_depth <= 8 is Sampled"
    same_arrays(results[2], results[0], "rows permuted")
    assert images[2] == images[0], "with subsample = 1 the forest does not depend on the order of the rows, nor on the grid"


# ---- 7. refusals ----

def test_the_calls_without_a_seed_are_refused_and_leave_everything_alone(torch_cuda, tmp_path):
    n, nfeat = 1300, 4
    x, y, w, cuts, _ = O.inputs(n, 304, nfeat, 32, 0)
    b = booster((), nfeat=nfeat)
    d = capi.DMatrix(x, missing=NAN)
    b.boost_trees_weighted(d, y, cuts, weights=w, rounds=2, max_depth=4, min_child_weight=0.0)      # a forest to leave alone
    before = saved(b, tmp_path)
    tx, ty = torch_cuda.from_numpy(x).cuda(), torch_cuda.from_numpy(y).cuda()
    dd = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=n, ncol=nfeat, missing=NAN)
    torch_cuda.cuda.synchronize()
    b.set_param("ohx_colsample_bynode", "0.5")
    for refused in (lambda: b.boost_trees(d, y, cuts, rounds=1, max_depth=3),
                    lambda: b.boost_trees_eval(d, y, cuts, rounds=1, max_depth=3),
                    lambda: b.boost_trees_weighted(d, y, cuts, weights=w, rounds=1, max_depth=3),
                    lambda: b.boost_trees_deep(d, y, cuts, weights=w, rounds=1, max_depth=10),
                    lambda: b.boost_trees_device(dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=3),
                    lambda: b.boost_trees_eval_device(dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=3),
                    lambda: b.boost_trees_weighted_device(dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=3),
                    lambda: b.boost_trees_deep_device(dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=10)):
        with pytest.raises(capi.OhxError, match="OHXBoosterBoostTreesSampled"):
            refused()
    assert saved(b, tmp_path) == before, "the calls without a seed"
    # through the C interface itself: no output is written
    ptr, vals = b._cuts(cuts)
    train, evals = np.full(3, -7.0), np.full(3, -7.0)
    run, best, added = C.c_int32(-7), C.c_int32(-7), C.c_uint64(77)
    rc = b.lib.OHXBoosterBoostTreesWeighted(b.handle, d.handle, y.ctypes.data, w.ctypes.data, n, None, None, None, 0, ptr.ctypes.data,
                                            vals.ctypes.data, 2, 3, 0.5, 1.0, 0.0, 0.0, 0, train.ctypes.data, evals.ctypes.data,
                                            C.byref(run), C.byref(best), C.byref(added))
    with pytest.raises(capi.OhxError, match="ohx_colsample_bynode"):
        capi.check(b.lib, rc)
    assert np.all(train == -7.0) and np.all(evals == -7.0) and run.value == -7 and best.value == -7 and added.value == 77
    # the refit chooses no split and is unaffected; a sampled call follows
    b.refit_leaves(d, y)
    before = saved(b, tmp_path)
    got = b.boost_trees_sampled(d, y, cuts, weights=w, rounds=1, max_depth=4, min_child_weight=0.0, seed=3)
    assert got["nodes_added"] > 0 and saved(b, tmp_path) != before
    done(b, [d, dd])


# ---- 8. deep levels with more open nodes than a batch holds ----

def test_more_open_nodes_at_a_level_than_a_batch_holds(torch_cuda, tmp_path):
    """Depth 16, one round of pseudo-Huber at the rows and weights of test_gpu_grow_mono.py's case: phase 0 of a deep level
    ranks the nodes of a second batch by their ids in the whole level, and phase 1 walks its slots in several chunks."""
    n, nfeat = 24000, 4
    x, y, _, cuts, _ = O.inputs(n, 263, nfeat, 16, 0)
    w = np.full(n, 128.0, F32)
    want = K.boost(0.75, 0.67, (), "pseudohuber", 1.0, 0.0, 0.0, "rmse", np.full(n, O.BASE, F32), x, NAN, y, w, cuts, nfeat, rounds=1,
                   max_depth=16, eta=0.125, lam=1.0, min_child_weight=0.0, seed=DRAW_SEED)
    assert max(o for o, _ in D.levels(want["trees"][0])) > synth.grow_deep_batch(), "a level of two batches"
    late = [e for e in want["draws"][0] if e["d"] >= 8 and e["free"] is not None and e["free"] not in e["node"]]
    assert len(late) > 100, "nodes of the deep levels whose best candidate is not their own"
    c = case("deep_sampled", n, nfeat, 16, 16, 0.75, 0.67, rounds=1, objective="pseudohuber")
    check(torch_cuda, tmp_path, c, want, x, y, w, cuts, None, "deep, two batches")
