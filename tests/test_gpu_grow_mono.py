""""ohx_monotone_constraints" on the GPU (csrc/grow_mono.hip, through XGBoosterSetParam and monotone_constraints= of the
Python binding).  Every array of every new tree, nodes_added, rounds_run and best_round are compared as integers or bit for
bit, both metric arrays with ==, and models byte for byte in all three formats.

The expected values are the restatement's (tests/grow_mono_support.py, written from the header) and, where the header
states an equality, another call on a twin booster.  The model of every case has no tree, so the margin a restatement
starts from is the model's base.  What a case is meant to reach - a tree that the constraints change, a level beyond 7,
more open nodes than a batch holds, a tree whose list lacks a constrained feature - is asserted from the restatement before
the GPU is asked.  gamma, lambda, min_child_weight and eta away from kind_kw's values: tests/test_gpu_grow_hyper.py."""
import ctypes as C

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_deep_support as D
from tests import grow_mono_support as M
from tests import grow_objective_support as O
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests.test_gpu_grow import held, same_new_trees
from tests.test_gpu_grow_eval import same_result, saved
from tests.test_gpu_grow_objective import KINDS, NFEAT, NAN, booster, call, done, kind_kw, same_arrays

pytestmark = pytest.mark.gpu

NAME = "ohx_monotone_constraints"
F32 = np.float32
SEED = 283
N_DEEP, N_LDS, HELD = 4097, 1300, 400     # a deep kind needs rows enough for level 8 to split,
N_DEEP_BAG = 8193                         # and twice as many where a bag keeps half of them and alpha closes small nodes
CONSTRAINTS = (1, 0, 0, -1)               # on the feature the labels bend in, and on the last


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def text(constraints):
    return "(" + ",".join(str(c) for c in constraints) + ")"


def params_of(constraints, objective="squarederror", alpha=0.0, m=0.0):
    return ((NAME, text(constraints)), ("ohx_objective", objective), ("ohx_huber_slope", "1.0"), ("ohx_reg_alpha", repr(float(alpha))),
            ("ohx_max_delta_step", repr(float(m))))


def restated(kind, constraints, objective="squarederror", alpha=0.0, m=0.0, n=None, seed=SEED, rounds=2, held_out=HELD, deep_depth=10,
             max_depth=None, nfeat=NFEAT, bins=32, **more):
    kw = kind_kw(kind, deep_depth)
    n = n or (N_DEEP_BAG if kind == "deep_sampled" else N_DEEP if kind == "deep" else N_LDS)
    return M.restated(tuple(constraints), objective, 1.0, alpha, m, "rmse", n, seed, max_depth or kw["max_depth"], bins=bins, nfeat=nfeat,
                      rounds=rounds, held_out=held_out, subsample=kw.get("subsample", 1.0), colsample=kw.get("colsample_bytree", 1.0),
                      draw_seed=kw.get("seed", 0), **more)


def check(torch, tmp_path, kind, want, x, y, w, cuts, ev, params, what, device=False, **kw):
    b = booster(params, nfeat=x.shape[1])
    got, mats = call(torch, b, kind, x, y, w, cuts, ev, device=device, **kw)
    same_result(got, want, what)
    same_new_trees(held(b, tmp_path)[0], want["trees"], 0, what)
    image = saved(b, tmp_path)
    done(b, mats)
    return got, image


# ---- 1. every kind, both forms, both objectives, with and without regularisation ----

@pytest.mark.parametrize("objective,alpha,m,device", (("squarederror", 0.0, 0.0, False), ("pseudohuber", 0.5, 0.5, True),
                                                      ("squarederror", 0.5, 0.5, True), ("pseudohuber", 0.0, 0.0, False)))
@pytest.mark.parametrize("kind", KINDS)
def test_constrained_trees_against_the_restatement(torch_cuda, tmp_path, kind, objective, alpha, m, device):
    x, y, w, cuts, ev, want = restated(kind, CONSTRAINTS, objective, alpha, m)
    *_, free = restated(kind, (), objective, alpha, m)
    assert not M.same_trees(want["all_trees"], free["all_trees"]), "the constraints change a tree"
    assert len(want["all_trees"]) == 2, "the second tree starts from fresh intervals"
    if "deep" in kind:      # (under alpha and the constraints the first tree of a bag may end at level 7; one of the two goes on)
        assert any(D.depth_of(t) > 8 and D.levels(t)[8][1] > 0 for t in want["all_trees"]), "level 8 splits: the hand-over"
    if "sampled" in kind:
        kw0 = kind_kw(kind)
        lists = [P.features(kw0["seed"], r, NFEAT, kw0["colsample_bytree"]) for r in range(2)]
        assert any(not {0, 3} <= set(kept) for kept in lists) and any({0, 3} & set(kept) for kept in lists), lists
    kw = dict(kind_kw(kind, 10), rounds=2)
    what = f"{kind}, {objective} at ({alpha}, {m})"
    if device:     # the device form, its parameters set by XGBoosterSetParam
        check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, params_of(CONSTRAINTS, objective, alpha, m), what, device=True, **kw)
    else:          # the host form, by the keyword arguments of the binding
        check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, (), what, objective=objective, huber_slope=1.0, reg_alpha=alpha,
              max_delta_step=m, monotone_constraints=CONSTRAINTS, **kw)


# ---- 2. rows, features and depths at their edges, the constraint on the last feature ----

# (rows, features, bins, kind, depth): a row alone, a wave less one, a wave, a wave and one, more than a block; a feature
# alone, 27 as the emulator has, 128 as the library takes; depths 1, 2, 6 and 8 on the LDS path, 9 and 12 on the deep one
SHAPES = ((1, 1, 8, "weighted", 1), (63, 3, 64, "weighted", 2), (64, 27, 16, "weighted", 6), (65, 128, 8, "weighted", 8),
          (4097, 1, 64, "weighted", 6), (4097, 3, 16, "weighted", 8), (4097, 27, 4, "deep", 9), (4097, 3, 16, "deep", 12))


@pytest.mark.parametrize("n,nfeat,bins,kind,depth", SHAPES)
def test_shapes_with_a_constraint_on_the_last_feature(torch_cuda, tmp_path, n, nfeat, bins, kind, depth):
    # (with many features of noise the last alone is rarely split on: x0, which the labels bend in, is constrained too)
    cons = (1,) if nfeat == 1 else (-1,) + (0,) * (nfeat - 2) + (1,)
    one = n == 1          # (a row alone needs a weight that is not 0: every weight 1)
    x, y, w, cuts, ev, want = restated(kind, cons, n=n, max_depth=depth, nfeat=nfeat, bins=bins, held_out=0, weighted=not one, seed=SEED + n)
    *_, free = restated(kind, (), n=n, max_depth=depth, nfeat=nfeat, bins=bins, held_out=0, weighted=not one, seed=SEED + n)
    if n >= 63:
        assert not M.same_trees(want["all_trees"], free["all_trees"]), "the constraint changes a tree"
    else:
        assert want["nodes_added"] == 2, "a root alone, twice"
    if depth > 8:
        assert D.depth_of(want["all_trees"][0]) > 8, "a level of the deep path"
    kw = dict(kind_kw(kind, depth), rounds=2, max_depth=depth)
    check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, ((NAME, text(cons)),), f"{n} x {nfeat}, depth {depth}", **kw)


# ---- 3. deep levels with more open nodes than a batch holds ----

def test_constrained_with_more_open_nodes_than_a_batch_holds(torch_cuda, tmp_path):
    """Depth 16, one round of pseudo-Huber, at the rows and weights of test_gpu_grow_reg.py's case: phase 1 of a deep level walks its slots in several
    chunks, and phase 0 reads the intervals of a second batch."""
    n, cons = 24000, (0, 0, 0, -1)     # (a constraint on x0 as well keeps every level of this tree below 600 open nodes)
    x, y, _, cuts, _ = O.inputs(n, 263, NFEAT, 16, 0)
    w = np.full(n, 128.0, F32)
    want = M.boost(cons, "pseudohuber", 1.0, 0.0, 0.0, "rmse", np.full(n, O.BASE, F32), x, NAN, y, w, cuts, NFEAT, rounds=1, max_depth=16,
                   eta=0.125, lam=1.0, min_child_weight=0.0)
    assert max(o for o, _ in D.levels(want["trees"][0])) > synth.grow_deep_batch(), "a level of two batches"
    narrowed = sum(1 for lo, hi in want["trees"][0]["intervals"] if lo > -M.INF or hi < M.INF)
    assert narrowed > 1000, "most nodes carry an interval that is not the whole line"
    kw = dict(kind_kw("deep", deep_depth=16), rounds=1)
    check(torch_cuda, tmp_path, "deep", want, x, y, w, cuts, None, params_of(cons, "pseudohuber"), "deep, two batches", **kw)


# ---- 4. NaN and -999 in a constrained column; rows permuted, and the grid ----

@pytest.mark.parametrize("kind", ("weighted", "deep"))
def test_missing_values_row_order_and_the_grid(torch_cuda, tmp_path, kind):
    n = N_DEEP if kind == "deep" else N_LDS
    x, y, w, _, ev = O.inputs(n, SEED + 1, NFEAT, 32, HELD)
    x = x.copy()
    x[::7, 0] = -999.0                 # a value like any other, far to the left; NaN (5 % of every column) is the missing one
    x[3::11, 3] = -999.0
    cuts = G.quantile_cuts(x, NAN, 32)
    assert np.isnan(x[:, 0]).any() and np.isnan(x[:, 3]).any() and (x[:, 0] == F32(-999.0)).any() and (x[:, 3] == F32(-999.0)).any()
    kw = dict(kind_kw(kind, 10), rounds=2)
    want = M.boost(CONSTRAINTS, "squarederror", 1.0, 0.0, 0.5, "rmse", np.full(n, O.BASE, F32), x, NAN, y, w, cuts, NFEAT, eval_set=ev,
                   eval_pred=np.full(HELD, O.BASE, F32), rounds=2, max_depth=kw["max_depth"], eta=0.125, lam=1.0, min_child_weight=0.0)
    assert any(t["default_left"][(t["left"] >= 0) & np.isin(t["feature"], (0, 3))].any() for t in want["trees"]), "missing goes left somewhere"
    params = params_of(CONSTRAINTS, m=0.5)
    _, image = check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, params, kind, **kw)
    order = np.random.default_rng(SEED + 2).permutation(n)
    b = booster(params)
    got, mats = call(torch_cuda, b, kind, np.ascontiguousarray(x[order]), y[order], w[order], cuts, ev, grid=True, **kw)
    same_result(got, want, kind + ", permuted")
    assert saved(b, tmp_path) == image, "permuted rows on a grid"
    done(b, mats)


# ---- 5. an equality that needs no restatement ----

@pytest.mark.parametrize("kind", KINDS)
def test_a_constraint_on_a_feature_without_cuts_changes_no_byte(torch_cuda, tmp_path, kind):
    """Under ohx_max_delta_step = 0.5 the regularised path takes the second gain form already; a constraint on a feature
    whose cut list is empty admits and refuses nothing and narrows no interval: the same bytes in all three formats.
    Then () and a list of zeros after an active list are the default."""
    n = N_DEEP if "deep" in kind else N_LDS
    x, y, w, _, ev = O.inputs(n, SEED + 3, NFEAT, 32, HELD)
    x = x.copy()
    x[:, 3] = F32(1.5)                 # one value: no cut
    cuts = G.quantile_cuts(x, NAN, 32)
    assert int(cuts[0][4]) == int(cuts[0][3])
    kw = dict(kind_kw(kind, 10), rounds=2)
    if "sampled" in kind:
        kw["colsample_bytree"] = 1.0   # (every tree sees the feature: the subsample alone makes the kind)
    images, results = [], []
    for params in ((("ohx_max_delta_step", "0.5"),), (("ohx_max_delta_step", "0.5"), (NAME, "(0,0,0,-1)"))):
        b = booster(params)
        got, mats = call(torch_cuda, b, kind, x, y, w, cuts, ev, **kw)
        results.append(got)
        images.append(saved(b, tmp_path))
        done(b, mats)
    same_arrays(results[1], results[0], kind)
    assert images[1] == images[0] and results[0]["nodes_added"] > 20, kind
    # the default's bytes: never set, set and taken back by (), set and taken back by zeros
    images, results = [], []
    for values in ((), ("(1,0,0,-1)", "()"), ("(1,0,0,-1)", "(0, 0, 0, 0)"), ("(1,0,0,-1)",)):
        b = booster()
        for v in values:
            b.set_param(NAME, v)
        got, mats = call(torch_cuda, b, kind, x, y, w, cuts, ev, **kw)
        results.append(got)
        images.append(saved(b, tmp_path))
        done(b, mats)
    for k in (1, 2):
        same_arrays(results[k], results[0], kind)
        assert images[k] == images[0], (kind, k)
    assert images[3] != images[0], "the active list changes the trees"


# ---- 6. the property ----

def monotone(values, c):
    return M.violations(values, c) == 0


def test_every_new_tree_and_the_margins_are_monotone(torch_cuda, tmp_path):
    """32 base rows, the constrained feature swept over every cut value and the midpoints between cuts.  Each new tree,
    walked on the host from the saved arrays, and the library's own margins are monotone with exact comparisons: float32
    addition is monotone in each argument, and all rows of one call share one summation order."""
    x, y, w, cuts, want = M.property_case(True)
    p = M.PROPERTY
    sweeps = M.property_sweeps(x, cuts)
    kw = dict(kind_kw("weighted"), rounds=p["rounds"], max_depth=p["max_depth"])
    margins = {}
    for constrained in (True, False):
        b = booster(((NAME, text(p["constraints"])),) if constrained else (), nfeat=p["nfeat"])
        got, mats = call(torch_cuda, b, "weighted", x, y, w, cuts, None, **kw)
        trees = held(b, tmp_path)[0]
        if constrained:
            same_new_trees(trees, want["trees"], 0, "the property's trees")
        for f, rows in sweeps.items():
            c = p["constraints"][f]
            r, k, ncol = rows.shape
            d = capi.DMatrix(np.ascontiguousarray(rows.reshape(r * k, ncol)), missing=NAN)
            margin = b.predict(d, option_mask=1).reshape(r, k)
            d.free()
            per_tree = [M.tree_values(t, rows) for t in trees]
            assert np.allclose(O.BASE + sum(v.astype(np.float64) for v in per_tree), margin, rtol=0, atol=1e-5), "the margins of these trees"
            margins[constrained, f] = (c, per_tree, margin)
        done(b, mats)
    for f in sweeps:
        c, per_tree, margin = margins[True, f]
        assert all(monotone(v, c) for v in per_tree), ("a new tree, walked on the host", f)
        assert monotone(margin, c), ("the library's margins", f)
    assert any(not monotone(v, c) for f in sweeps for c, per_tree, _ in (margins[False, f],) for v in per_tree), "a free tree is not"


# ---- 7. refusals ----

def test_refusals_leave_the_forest_and_the_outputs_alone(torch_cuda, tmp_path):
    x, y, w, cuts, ev = O.inputs(N_LDS, SEED + 4, NFEAT, 32, HELD)
    kw = dict(kind_kw("weighted"), rounds=2)
    b = booster()
    d = capi.DMatrix(x, missing=NAN)
    b.boost_trees_weighted(d, y, cuts, weights=w, **kw)      # a forest to leave alone
    before = saved(b, tmp_path)
    tx, ty = torch_cuda.from_numpy(x).cuda(), torch_cuda.from_numpy(y).cuda()
    dd = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=N_LDS, ncol=NFEAT, missing=NAN)
    torch_cuda.cuda.synchronize()
    b.set_param(NAME, "(0,0,0,1)")
    for refused in (lambda: b.boost_trees(d, y, cuts, rounds=1, max_depth=3),
                    lambda: b.boost_trees_eval(d, y, cuts, rounds=1, max_depth=3),
                    lambda: b.boost_trees_device(dd, ty.data_ptr(), N_LDS, cuts, rounds=1, max_depth=3),
                    lambda: b.boost_trees_eval_device(dd, ty.data_ptr(), N_LDS, cuts, rounds=1, max_depth=3),
                    lambda: b.refit_leaves(d, y),
                    lambda: b.refit_leaves_device(dd, ty.data_ptr(), N_LDS)):
        with pytest.raises(capi.OhxError, match="OHXBoosterBoostTreesWeighted"):
            refused()
    assert saved(b, tmp_path) == before, "the calls that keep row counts, and the refit"
    # more entries than the booster has features: every call with row weights, through the C interface itself
    b.set_param(NAME, "(0,0,0,0,1)")
    ptr, vals = b._cuts(cuts)
    train, evals = np.full(3, -7.0), np.full(3, -7.0)
    run, best, added = C.c_int32(-7), C.c_int32(-7), C.c_uint64(77)
    rc = b.lib.OHXBoosterBoostTreesWeighted(b.handle, d.handle, y.ctypes.data, w.ctypes.data, N_LDS, None, None, None, 0, ptr.ctypes.data,
                                            vals.ctypes.data, 2, 3, 0.5, 1.0, 0.0, 0.0, 0, train.ctypes.data, evals.ctypes.data,
                                            C.byref(run), C.byref(best), C.byref(added))
    with pytest.raises(capi.OhxError, match=NAME):
        capi.check(b.lib, rc)
    assert np.all(train == -7.0) and np.all(evals == -7.0) and run.value == -7 and best.value == -7 and added.value == 77
    for kind in KINDS:
        with pytest.raises(capi.OhxError, match=NAME):
            getattr(b, "boost_trees_" + kind)(d, y, cuts, weights=w, **dict(kind_kw(kind, 10), rounds=1))
        with pytest.raises(capi.OhxError, match=NAME):
            getattr(b, "boost_trees_" + kind + "_device")(dd, ty.data_ptr(), N_LDS, cuts, **dict(kind_kw(kind, 10), rounds=1))
    assert saved(b, tmp_path) == before, "too many entries"
    # a refused value leaves the handle's setting: still too many
    with pytest.raises(capi.OhxError, match=NAME):
        b.set_param(NAME, "(2)")
    with pytest.raises(capi.OhxError, match=NAME):
        b.boost_trees_weighted(d, y, cuts, weights=w, **kw)
    # a valid call follows: as many entries as features, and the trees are the restatement's on top of the forest
    b.set_param(NAME, "(0,0,0,0)")
    b.boost_trees(d, y, cuts, rounds=1, max_depth=3)         # all zeros is the default: the count call is no refusal
    before = saved(b, tmp_path)
    # a root with H == 0 under a bag still says "bag"
    b.set_param(NAME, text(CONSTRAINTS))
    with pytest.raises(capi.OhxError, match="bag"):
        b.boost_trees_sampled(d, y, cuts, weights=np.zeros(N_LDS, F32), subsample=0.5, colsample_bytree=0.5, seed=3, rounds=1, max_depth=3)
    assert saved(b, tmp_path) == before, "an empty bag"
    got = b.boost_trees_weighted(d, y, cuts, weights=w, **kw)
    assert got["nodes_added"] > 0 and saved(b, tmp_path) != before, "a valid call after the refusals"
    done(b, [d, dd])
