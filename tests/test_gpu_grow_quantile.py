"""Quantile boosting on the GPU (csrc/grow_quantile.hip; "ohx_objective" = quantile, "ohx_quantile_alpha" and
"ohx_eval_metric" = quantile of XGBoosterSetParam).  Every array of every new tree, nodes_added, rounds_run and best_round
are compared as integers or bit for bit, both metric arrays with ==, the margin of the saved model bit for bit, and models
byte for byte in all three formats.

The expected values are the restatement's (tests/grow_quantile_support.py, written from the header: the leaf by sorting keys
and cumulating weights in Python integers).  The model of the cases of sections 1 to 8 has no tree, so the margin a
restatement starts from is the model's base; section 10 boosts a forest that has trees, twice on one handle.  Section 9 takes
every row loop of the file through more than two trips, the trips computed from the launch shape the library exports
(synth.grow_quantile_plan); section 11 grows quantile trees away from the default gamma, lambda, min_child_weight and eta
and puts the library's own trees under the exact audit of tests/grow_audit_support.py and its leaf check for quantile trees;
section 12 is a tie of the pinball metric under the stop rule.  What a case is meant to reach - more leaves than one, two or
three groups of the select hold, a second trip, a split that min_child_weight moved - is asserted from the restatement
before the GPU is asked.  No test asserts a duration."""
import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_audit_support as A
from tests import grow_objective_support as O
from tests import grow_quantile_support as Q
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests import grow_weighted_support as W
from tests import helpers
from tests.test_gpu_grow import held, same_new_trees
from tests.test_gpu_grow_eval import same_result, saved
from tests.test_gpu_grow_hyper import expected_images
from tests.test_gpu_grow_objective import N, ROWS_PAST_A_STRIDE, booster, call, done

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = np.float32
SAMPLING = dict(subsample=0.5, colsample_bytree=0.5, seed=11)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def check(torch, tmp_path, kind, want, x, y, w, cuts, ev, params, what, device=False, base=Q.BASE, missing=NAN, **kw):
    """One call on a fresh booster against the restatement: the result, the new trees, the margin of the saved model by
    XGBoosterPredict against the call's pred.  -> (the result, the three images)."""
    b = booster(params, nfeat=x.shape[1], base=base)
    if np.isnan(missing):
        got, mats = call(torch, b, kind, x, y, w, cuts, ev, device=device, **kw)
    else:                                     # the host form with a missing value that is a number
        d = capi.DMatrix(x, missing=missing)
        ed = capi.DMatrix(ev[0], missing=ev[1]) if ev is not None else None
        got = getattr(b, "boost_trees_" + kind)(d, y, cuts, weights=w, eval_set=(ed, ev[2], ev[3]) if ev is not None else None, **kw)
        mats = [m for m in (d, ed) if m is not None]
    same_result(got, want, what)
    same_new_trees(held(b, tmp_path)[0], want["trees"], 0, what)
    image = saved(b, tmp_path)
    d = capi.DMatrix(x, missing=missing)
    assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want["pred"])), (what, "XGBoosterPredict")
    done(b, mats + [d])
    return got, image


def leaves_of(t):
    return int(np.count_nonzero(t["left"] < 0))


# ---- 1. against the restatement, over the shapes ----

# kind, device form, rows, features, depth, rounds, alpha, eta, weights, missing, held-out rows, patience
SHAPES = (
    ("weighted", False, 1, 1, 1, 1, 0.5, 1.0, False, NAN, 0, 0),
    ("weighted", True, 63, 3, 2, 2, 2.0 ** -10, 0.125, True, NAN, 0, 0),
    ("weighted", False, 64, 1, 6, 5, 0.05, 0.125, True, -999.0, 0, 0),
    ("weighted", True, 65, 27, 8, 1, 0.95, 1.0, False, NAN, 0, 0),
    ("weighted", False, 4097, 3, 6, 2, 1.0 - 2.0 ** -10, 0.125, True, NAN, 1300, 0),
    ("weighted", True, 4097, 27, 8, 2, 0.5, 0.125, True, NAN, 1300, 2),
    ("weighted", False, 4097, 3, 1, 5, 0.95, 1.0, True, -999.0, 0, 0),
    ("sampled", False, 63, 3, 2, 2, 0.5, 0.125, False, NAN, 0, 0),
    ("sampled", True, 64, 27, 6, 1, 0.05, 1.0, True, NAN, 0, 0),
    ("sampled", False, 65, 3, 8, 5, 0.95, 0.125, True, -999.0, 0, 0),
    ("sampled", True, 4097, 3, 6, 2, 0.5, 0.125, True, NAN, 1300, 2),
    ("sampled", False, 4097, 27, 8, 2, 1.0 - 2.0 ** -10, 1.0, False, NAN, 1300, 0),
    ("sampled", True, 4097, 3, 2, 5, 2.0 ** -10, 0.125, True, NAN, 0, 0),
)


def shape_id(s):
    return "-".join(str(v) for v in (s[0], "device" if s[1] else "host", s[2], s[3], "d%d" % s[4], "r%d" % s[5], "a%g" % s[6], "eta%g" % s[7],
                                     "w" if s[8] else "now", "nan" if np.isnan(s[9]) else "m999", "held%d" % s[10], "p%d" % s[11]))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_against_the_restatement(torch_cuda, tmp_path, shape):
    kind, device, n, nfeat, depth, rounds, alpha, eta, weighted, missing, held_out, patience = shape
    sampling = SAMPLING if kind == "sampled" else {}
    x, y, w, cuts, ev, want = Q.restated("quantile", alpha, n, 3210 + n + nfeat, depth, nfeat=nfeat, rounds=rounds, held_out=held_out,
                                         patience=patience, subsample=sampling.get("subsample", 1.0),
                                         colsample=sampling.get("colsample_bytree", 1.0), draw_seed=sampling.get("seed", 0), eta=eta,
                                         weighted=weighted, missing=missing)
    if n >= 4097 and depth >= 6:
        assert leaves_of(want["all_trees"][0]) > 8 and len(want["leaf_keys"][0]) == leaves_of(want["all_trees"][0])
    if weighted and n >= 63:
        assert np.count_nonzero(w == 0.0) > 0, "zero weights among the rows"
    kw = dict(rounds=rounds, max_depth=depth, eta=eta, reg_lambda=1.0, min_child_weight=0.0, patience=patience, **sampling)
    assert not device or np.isnan(missing), "the device form's cases use NaN"
    # the host form sets the handle by the binding's keywords, the device form by XGBoosterSetParam
    if device:
        params = (("ohx_objective", "quantile"), ("ohx_quantile_alpha", repr(float(alpha))))
        check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, params, shape_id(shape), device=True, **kw)
    else:
        check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, (), shape_id(shape), missing=missing, objective="quantile",
              quantile_alpha=alpha, **kw)


# ---- 2. more leaves than one, and than three, groups of the select hold ----

@pytest.mark.parametrize("n,seed,least,most", ((1200, 3221, 65, 192), (20000, 3222, 193, 256)))
def test_every_leaf_group_of_the_select(torch_cuda, tmp_path, n, seed, least, most):
    x, y, w, cuts, ev, want = Q.restated("quantile", 0.5, n, seed, 8, nfeat=3, rounds=1, mcw=0.0, bins=64)
    leaves = leaves_of(want["trees"][0])
    assert least <= leaves <= most, leaves
    check(torch_cuda, tmp_path, "weighted", want, x, y, w, cuts, None, (("ohx_objective", "quantile"),), f"{leaves} leaves", rounds=1,
          max_depth=8, eta=0.125, reg_lambda=1.0, min_child_weight=0.0)


# ---- 3. the crafted leaves, each the rows of one leaf of a depth-1 tree ----

@pytest.mark.parametrize("alpha", Q.ALPHAS)
def test_crafted_leaves(torch_cuda, tmp_path, alpha):
    split = 0
    cuts = (np.asarray([0, 1], np.uint64), np.asarray([0.5], F32))
    for name, r, wl in Q.crafted_leaves():
        # the crafted rows at x = 0, and beside them forty rows far on the other side of the margin at x = 1
        x = np.concatenate([np.zeros(len(r), F32), np.ones(40, F32)]).reshape(-1, 1)
        y = np.concatenate([r, np.full(40, -100.0, F32)])
        w = np.concatenate([wl, np.ones(40, F32)])
        want = Q.boost("quantile", alpha, np.zeros(len(y), F32), x, NAN, y, w, cuts, 1, rounds=1, max_depth=1, eta=1.0,
                       min_child_weight=0.0)
        t = want["trees"][0]
        if len(t["left"]) == 3:
            split += 1
            rows = np.arange(len(r))
            k = Q.leaf_key(Q.keys(r), W.hess_fixed(wl), Q.alpha_q(alpha))
            assert k is not None and helpers.bits(t["value"][1:2])[0] == helpers.bits(np.asarray([Q.unkey(k)], F32))[0], name
            assert np.all(want["pos"][0][rows] == 1)
        check(torch_cuda, tmp_path, "weighted", want, x, y, w, cuts, None, (), f"{name} at {alpha}", base=0.0, rounds=1, max_depth=1,
              eta=1.0, min_child_weight=0.0, objective="quantile", quantile_alpha=alpha)
    assert split >= 4, "most crafted leaves stand alone on their node"


# ---- 4. the order of the rows ----

@pytest.mark.parametrize("kind", ("weighted", "sampled"))
def test_permuted_rows_give_the_same_bytes(torch_cuda, tmp_path, kind):
    sampling = dict(colsample_bytree=0.5, seed=11) if kind == "sampled" else {}      # (a bag is drawn by row index)
    x, y, w, cuts, ev, want = Q.restated("quantile", 0.05, 4097, 3230, 6, nfeat=4, rounds=2, held_out=700, colsample=sampling.get("colsample_bytree", 1.0),
                                         draw_seed=sampling.get("seed", 0))
    kw = dict(rounds=2, max_depth=6, eta=0.125, min_child_weight=0.0, **sampling)
    params = (("ohx_objective", "quantile"), ("ohx_quantile_alpha", "0.05"))
    _, image = check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, params, kind, **kw)
    order = np.random.default_rng(3231).permutation(len(y))
    b = booster(params, nfeat=4)
    got, mats = call(torch_cuda, b, kind, np.ascontiguousarray(x[order]), y[order], w[order], cuts, ev, grid=True, **kw)
    same_result(got, want, kind + ", permuted")
    assert saved(b, tmp_path) == image, "permuted rows on a grid"
    done(b, mats)


# ---- 5. the coverage property on the device's own leaves ----

@pytest.mark.parametrize("alpha", Q.ALPHAS)
def test_every_leaf_covers_its_quantile(torch_cuda, tmp_path, alpha):
    x, y, w, cuts, ev, want = Q.restated("quantile", alpha, 4097, 3240, 6, nfeat=3, rounds=1, eta=1.0)
    b = booster((("ohx_objective", "quantile"), ("ohx_quantile_alpha", repr(float(alpha)))), nfeat=3)
    got, mats = call(torch_cuda, b, "weighted", x, y, w, cuts, None, rounds=1, max_depth=6, eta=1.0, min_child_weight=0.0)
    trees, _ = held(b, tmp_path)
    same_new_trees(trees, want["trees"], 0, "structure")
    pos, hb = want["pos"][0], want["hessians"][0]
    base = np.full(len(y), Q.BASE, F32)
    k = Q.keys(y - base)
    value = np.asarray(want["trees"][0]["value"], F32)       # (bit for bit the device's: same_new_trees)
    aq, seen = Q.alpha_q(alpha), 0
    for p in np.flatnonzero(want["trees"][0]["left"] < 0):
        rows = pos == p
        if int(hb[rows].astype(object).sum()) == 0:
            continue
        kstar = int(Q.keys(value[p:p + 1])[0])                # eta = 1: the value is q_p itself
        assert Q.covers(k[rows][hb[rows] > 0], hb[rows][hb[rows] > 0], aq, kstar), (alpha, p)
        seen += 1
    assert seen > 8
    # the device's own pred: the margin of the new model is base + value[pos], one float32 add a row
    d = mats[0]
    assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(base + value[pos]))
    # and in the large the quantile is met: about alpha of the weight lies at or below the new margin
    mq = W.hess_fixed(w).astype(np.float64)
    frac = mq[y <= base + value[pos]].sum() / mq.sum()
    assert abs(frac - float(F32(alpha))) < 0.05, (alpha, frac)
    done(b, mats)


# ---- 6. the metric ----

@pytest.mark.parametrize("patience", (0, 2))
@pytest.mark.parametrize("objective", ("squarederror", "pseudohuber", "quantile"))
def test_the_quantile_metric_with_each_objective(torch_cuda, tmp_path, objective, patience):
    x, y, w, cuts, ev, want = Q.restated(objective, 0.95, 4097, 3250, 6, nfeat=4, rounds=3, held_out=1300, patience=patience,
                                         metric="quantile", slope=3.7, subsample=0.5, colsample=0.5, draw_seed=11)
    assert want["eval_sums"][0] > 1 << 64 and len(set(want["eval_sums"])) > 1
    params = (("ohx_objective", objective), ("ohx_quantile_alpha", "0.95"), ("ohx_huber_slope", "3.7"), ("ohx_eval_metric", "quantile"))
    check(torch_cuda, tmp_path, "sampled", want, x, y, w, cuts, ev, params, f"{objective}, patience {patience}", device=patience == 2,
          rounds=3, max_depth=6, eta=0.125, min_child_weight=0.0, patience=patience, **SAMPLING)


def test_the_quantile_metric_on_a_deep_call(torch_cuda, tmp_path):
    x, y, w, cuts, ev, want = Q.restated("squarederror", 0.05, 4097, 3251, 10, nfeat=4, rounds=2, held_out=1300, patience=0,
                                         metric="quantile")
    from tests import grow_deep_support as D
    assert D.depth_of(want["trees"][0]) > 8
    check(torch_cuda, tmp_path, "deep", want, x, y, w, cuts, ev, (("ohx_eval_metric", "quantile"), ("ohx_quantile_alpha", "0.05")),
          "deep, squared error", rounds=2, max_depth=10, eta=0.125, min_child_weight=0.0)


# ---- 7. refusals, and the defaults afterwards ----

def test_refusals_then_the_default_call(torch_cuda, tmp_path):
    n, nfeat = 4097, 4
    x, y, w, cuts, ev, want = Q.restated("squarederror", 0.5, n, 3260, 6, nfeat=nfeat, rounds=2, held_out=700)
    kw = dict(rounds=2, max_depth=6, eta=0.125, min_child_weight=0.0)
    b = booster(nfeat=nfeat)
    d = capi.DMatrix(x, missing=NAN)
    ed = capi.DMatrix(ev[0], missing=NAN)
    before = saved(b, tmp_path)
    tx, ty = torch_cuda.from_numpy(x).cuda(), torch_cuda.from_numpy(y).cuda()
    dd = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=n, ncol=nfeat, missing=NAN)
    torch_cuda.cuda.synchronize()
    b.set_param("ohx_objective", "quantile")

    def refused(match, fn, *a, **k):
        with pytest.raises(capi.OhxError, match=match):
            fn(*a, **k)
        assert saved(b, tmp_path) == before, match

    # the calls that keep row counts, and the refit: as under pseudohuber
    refused("OHXBoosterBoostTreesWeighted", b.boost_trees, d, y, cuts, rounds=1, max_depth=3)
    refused("OHXBoosterBoostTreesWeighted", b.boost_trees_eval, d, y, cuts, rounds=1, max_depth=3)
    refused("OHXBoosterBoostTreesWeighted", b.boost_trees_device, dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=3)
    refused("OHXBoosterBoostTreesWeighted", b.boost_trees_eval_device, dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=3)
    refused("quantile", b.refit_leaves, d, y)
    refused("quantile", b.refit_leaves_device, dd, ty.data_ptr(), n)
    # the Deep forms at any depth
    for depth in (3, 8, 12):
        refused("OHXBoosterBoostTreesSampled", b.boost_trees_deep, d, y, cuts, weights=w, rounds=1, max_depth=depth)
        refused("OHXBoosterBoostTreesSampled", b.boost_trees_deep_sampled, d, y, cuts, weights=w, rounds=1, max_depth=depth, **SAMPLING)
    refused("OHXBoosterBoostTreesSampled", b.boost_trees_deep_device, dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=12)
    refused("OHXBoosterBoostTreesSampled", b.boost_trees_deep_sampled_device, dd, ty.data_ptr(), n, cuts, rounds=1, max_depth=12, **SAMPLING)
    # every setting that replaces the pair path's split kernels; the message names what to unset
    for name, value, reset in (("ohx_reg_alpha", "0.5", "0"), ("ohx_max_delta_step", "0.7", "0"),
                               ("ohx_monotone_constraints", "(1,0,-1)", "()"), ("ohx_colsample_bylevel", "0.5", "1"),
                               ("ohx_colsample_bynode", "0.5", "1")):
        b.set_param(name, value)
        refused(name, b.boost_trees_sampled, d, y, cuts, weights=w, rounds=1, max_depth=3, **SAMPLING)
        if "colsample" not in name:            # (the weighted call refuses those two whatever the objective)
            refused(name, b.boost_trees_weighted, d, y, cuts, weights=w, rounds=1, max_depth=3)
        b.set_param(name, reset)
    # the metric is accepted wherever mae is, and refused where mae is
    b.set_param("ohx_objective", "squarederror")
    b.set_param("ohx_eval_metric", "quantile")
    refused("ohx_eval_metric", b.boost_trees, d, y, cuts, rounds=1, max_depth=3)
    b.set_param("ohx_eval_metric", "rmse")
    # a default call follows: the bytes of the Weighted call as the existing restatement has them
    got = b.boost_trees_weighted(d, y, cuts, weights=w, eval_set=(ed, ev[2], ev[3]), **kw)
    same_result(got, want, "the default call after the refusals")
    same_new_trees(held(b, tmp_path)[0], want["trees"], 0, "the default call after the refusals")
    done(b, [d, ed, dd])


def test_setting_squarederror_again_restores_the_default_bytes(torch_cuda, tmp_path):
    x, y, w, cuts, ev, want = Q.restated("squarederror", 0.5, 4097, 3260, 6, nfeat=4, rounds=2, held_out=700)
    kw = dict(rounds=2, max_depth=6, eta=0.125, min_child_weight=0.0)
    plain = booster()
    _, mats = call(torch_cuda, plain, "weighted", x, y, w, cuts, ev, **kw)
    image = saved(plain, tmp_path)
    done(plain, mats)
    b = booster((("ohx_objective", "quantile"), ("ohx_quantile_alpha", "0.05")))
    _, mats = call(torch_cuda, b, "weighted", x, y, w, cuts, ev, **kw)
    assert saved(b, tmp_path) != image, "the loss is another one"
    b.set_param("ohx_objective", "squarederror")
    b.free()
    b = booster((("ohx_objective", "quantile"), ("ohx_quantile_alpha", "0.05")))
    b.set_param("ohx_objective", "squarederror")
    got, more = call(torch_cuda, b, "weighted", x, y, w, cuts, ev, **kw)
    same_result(got, want, "reset")
    assert saved(b, tmp_path) == image
    done(b, mats + more)


# ---- 8. the three formats ----

def test_the_three_formats_round_trip(torch_cuda, tmp_path):
    x, y, w, cuts, ev, want = Q.restated("quantile", 0.95, 4097, 3270, 6, nfeat=3, rounds=2)
    _, images = check(torch_cuda, tmp_path, "weighted", want, x, y, w, cuts, None, (), "formats", rounds=2, max_depth=6, eta=0.125,
                      min_child_weight=0.0, objective="quantile", quantile_alpha=0.95)
    d = capi.DMatrix(x, missing=NAN)
    for ext, image in zip(("json", "ubj", "bin"), images):
        path = str(tmp_path / f"grown.{ext}")
        with open(path, "wb") as f:
            f.write(image)
        again = capi.Booster(model_file=path)
        back, _ = held(again, tmp_path, f"back_{ext}.json")
        same_new_trees(back, want["trees"], 0, ext)
        assert saved(again, tmp_path) == images, (ext, "a loaded image saves as all three again")
        assert np.array_equal(helpers.bits(again.predict(d, option_mask=1)), helpers.bits(want["pred"])), ext
        again.free()
    d.free()


# ---- 9. more rows than two trips of every row loop of the file ----

def long_n(torch):
    """ROWS_PAST_A_STRIDE, or more where the device's CU count asks for more: past two trips of the pass kernel at the depth
    that gives it the most blocks, and past one trip of the streaming grids (the pair kernel and both metric kernels)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = ROWS_PAST_A_STRIDE
    full = [synth.grow_quantile_plan(1 << 30, depth, cus) for depth in (6, 8)]
    need = max(max(2 * p["pass_blocks"] * p["pass_block_rows"] for p in full), full[0]["row_blocks"] * synth.grow_plan(1 << 30, 3, 0, 6, cus)["block_rows"])
    if n <= need:
        n = need + 4097 + 64 + 1
    for depth in (6, 8):
        p, g = synth.grow_quantile_plan(n, depth, cus), synth.grow_plan(n, 3, 0, depth, cus)
        assert n % 64 != 0 and n > 2 * p["pass_blocks"] * p["pass_block_rows"] and n > p["row_blocks"] * 256, (n, p)
        assert g["row_blocks"] == p["row_blocks"] and g["block_rows"] == 256 and p["groups"] == (1, 4)[depth == 8]
        print("cus", cus, "rows", n, "depth", depth, p)
    return n


# kind, depth, alpha, more than this many leaves, held-out rows
LONG = (("weighted", 6, 0.05, 32, 0), ("weighted", 8, 0.05, 128, 0), ("sampled", 8, 0.95, 16, 1300))


@pytest.mark.parametrize("kind,depth,alpha,least,held_out", LONG, ids=lambda v: str(v))
def test_more_rows_than_two_trips_of_the_select(torch_cuda, tmp_path, kind, depth, alpha, least, held_out):
    """One round over weighted rows, zeros among them.  At depth 6 one group holds more than 32 leaves and the pass kernel
    has the most blocks it ever has; at depth 8 more than 128 leaves stand in three groups or four and a group has a quarter
    of the blocks, so a block takes eight trips and more; the Sampled call adds a bag whose last word is not full (its tree
    keeps two features of three and has few leaves: one group)."""
    n = long_n(torch_cuda)
    sampling = SAMPLING if kind == "sampled" else {}
    x, y, w, cuts, ev, want = Q.restated("quantile", alpha, n, 3308, depth, nfeat=3, rounds=1, mcw=0.0, held_out=held_out,
                                         subsample=sampling.get("subsample", 1.0), colsample=sampling.get("colsample_bytree", 1.0),
                                         draw_seed=sampling.get("seed", 0))
    leaves = leaves_of(want["trees"][0])
    assert leaves > least and len(want["leaf_keys"][0]) == leaves, leaves
    assert np.count_nonzero(w == 0.0) > n // 10, "rows of weight 0 among them"
    if kind == "sampled":
        assert 0 < np.count_nonzero(want["hessians"][0]) < np.count_nonzero(w) and not P.bag(11, 0, n, 0.5).all()
    params = (("ohx_objective", "quantile"), ("ohx_quantile_alpha", repr(float(alpha))))
    check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, params, f"{kind}, depth {depth}, {n} rows, {leaves} leaves", rounds=1,
          max_depth=depth, eta=0.125, reg_lambda=1.0, min_child_weight=0.0, **sampling)


def test_the_quantile_metric_past_one_stride_of_the_streaming_grids(torch_cuda, tmp_path):
    """test_gpu_grow_reg.test_rows_past_one_stride_of_the_streaming_grids for the metric its table does not hold: both metric
    kernels of the file take a second trip over the training rows and over as many held-out rows; squared error, depth 3."""
    n = long_n(torch_cuda)
    x, y, w, _, ev = O.inputs(n, 272, 4, 8, n)
    cuts = G.quantile_cuts(x[:N], NAN, 16)
    assert n % 64 != 0 and len(ev[2]) == n
    want = Q.boost("squarederror", 0.95, np.full(n, Q.BASE, F32), x, NAN, y, w, cuts, 4, eval_set=ev, eval_pred=np.full(n, Q.BASE, F32),
                   rounds=2, max_depth=3, eta=0.125, lam=1.0, min_child_weight=0.0, metric="quantile")
    assert len(set(want["train_sums"])) == 3 and len(set(want["eval_sums"])) == 3
    params = (("ohx_eval_metric", "quantile"), ("ohx_quantile_alpha", "0.95"))
    b = booster(params, nfeat=4)
    got, mats = call(torch_cuda, b, "weighted", x, y, w, cuts, ev, rounds=2, max_depth=3, eta=0.125, reg_lambda=1.0, min_child_weight=0.0)
    same_result(got, want, "long rows, the quantile metric")
    same_new_trees(held(b, tmp_path)[0], want["trees"], 0, "long rows, the quantile metric")
    done(b, mats)


# ---- 10. a forest that already has trees, and a handle used twice ----

def second_call(alpha, first, x, y, w, cuts, ev, depth):
    """Two more sampled rounds at `alpha` on the margins `first` left: the draws are those of trees 2 and 3."""
    return Q.boost("quantile", alpha, first["pred"], x, NAN, y, w, cuts, x.shape[1], eval_set=ev, eval_pred=first["eval_pred"], rounds=2,
                   patience=0, max_depth=depth, eta=0.125, lam=1.0, gamma=0.0, min_child_weight=0.0, subsample=SAMPLING["subsample"],
                   colsample_bytree=SAMPLING["colsample_bytree"], seed=SAMPLING["seed"], tree0=2)


def after_both_calls(torch, tmp_path, b, x, want1, want2, got1, got2, what):
    same_result(got1, want1, what + ", call 1")
    same_result(got2, want2, what + ", call 2")
    trees, _ = held(b, tmp_path)
    assert len(trees) == 4
    same_new_trees(trees[:2], want1["trees"], 0, what + ", the trees of call 1")
    same_new_trees(trees, want2["trees"], 2, what + ", the trees of call 2")
    assert saved(b, tmp_path) == expected_images(tmp_path, want1["trees"] + want2["trees"]), (what, "the bytes of a model that holds the four restated trees")
    d = capi.DMatrix(x, missing=NAN)
    assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want2["pred"])), (what, "XGBoosterPredict")
    return d


@pytest.mark.parametrize("depths", ((8, 3), (3, 8)), ids=("deep-then-shallow", "shallow-then-deep"))
def test_two_quantile_calls_on_one_handle(torch_cuda, tmp_path, depths):
    """alpha 0.05 then 0.95 set by XGBoosterSetParam, depth 8 then 3 or 3 then 8: the residuals of call 2 come from margins the
    library walked for itself, its draws are those of rounds 2 and 3, and the select's buffers, allocated once a handle, serve a
    grid of four leaf groups and one of one."""
    assert A.NFEAT == 4, "expected_images is written for four features"
    x, y, w, cuts, ev, want1 = Q.restated("quantile", 0.05, 4097, 3320, depths[0], nfeat=4, rounds=2, held_out=700, subsample=SAMPLING["subsample"],
                                          colsample=SAMPLING["colsample_bytree"], draw_seed=SAMPLING["seed"])
    want2 = second_call(0.95, want1, x, y, w, cuts, ev, depths[1])
    deep = (want1 if depths[0] == 8 else want2)["trees"][0]
    assert leaves_of(deep) > 64, "more leaves than a group holds: the other call's grid has one group"
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    assert synth.grow_quantile_plan(4097, 8, cus)["groups"] == 4 and synth.grow_quantile_plan(4097, 3, cus)["groups"] == 1
    assert not np.array_equal(P.bag(SAMPLING["seed"], 2, len(y), 0.5), P.bag(SAMPLING["seed"], 0, len(y), 0.5)), "round 2 draws another bag"
    assert not np.array_equal(want2["preds"][0], np.full(len(y), Q.BASE, F32)), "call 2 starts from no base"
    kw = dict(rounds=2, eta=0.125, reg_lambda=1.0, min_child_weight=0.0, patience=0, **SAMPLING)
    b = booster((("ohx_objective", "quantile"), ("ohx_quantile_alpha", "0.05")), nfeat=4)
    got1, mats = call(torch_cuda, b, "sampled", x, y, w, cuts, ev, max_depth=depths[0], **kw)
    b.set_param("ohx_quantile_alpha", "0.95")
    got2, more = call(torch_cuda, b, "sampled", x, y, w, cuts, ev, device=True, max_depth=depths[1], **kw)
    d = after_both_calls(torch_cuda, tmp_path, b, x, want1, want2, got1, got2, f"depths {depths}")
    done(b, mats + more + [d])


def test_quantile_rounds_on_top_of_squared_error_trees(torch_cuda, tmp_path):
    """Two squared-error rounds through the pair kernels ("ohx_grow_pairs" = on), then two quantile rounds on the same handle."""
    x, y, w, cuts, ev, want1 = O.restated("squarederror", 1.0, 4097, 3321, 6, bins=32, nfeat=4, rounds=2, held_out=700,
                                          subsample=SAMPLING["subsample"], colsample=SAMPLING["colsample_bytree"], draw_seed=SAMPLING["seed"])
    want2 = second_call(0.95, want1, x, y, w, cuts, ev, 6)
    assert leaves_of(want2["trees"][0]) > 8 and len(want2["leaf_keys"][0]) == leaves_of(want2["trees"][0])
    kw = dict(rounds=2, max_depth=6, eta=0.125, reg_lambda=1.0, min_child_weight=0.0, patience=0, **SAMPLING)
    b = booster((("ohx_grow_pairs", "on"),), nfeat=4)
    got1, mats = call(torch_cuda, b, "sampled", x, y, w, cuts, ev, device=True, **kw)
    b.set_param("ohx_objective", "quantile")
    b.set_param("ohx_quantile_alpha", "0.95")
    got2, more = call(torch_cuda, b, "sampled", x, y, w, cuts, ev, **kw)
    d = after_both_calls(torch_cuda, tmp_path, b, x, want1, want2, got1, got2, "squared error, then quantile")
    done(b, mats + more + [d])


# ---- 11. off the default gamma, lambda, min_child_weight and eta, and under the exact audit ----

def q_call(torch, case, x, y, w, cuts, ev, device):
    """One call of a case of grow_audit_support.Q_CASES on a booster without trees -> (the booster, the result, the matrices).
    The device form sets the handle by XGBoosterSetParam, the host form by the binding's keywords."""
    kw = A.q_hyper(case)
    if device:
        b = booster((("ohx_objective", "quantile"), ("ohx_quantile_alpha", repr(float(case[2])))), nfeat=A.NFEAT)
    else:
        b = booster(nfeat=A.NFEAT)
        kw.update(objective="quantile", quantile_alpha=case[2])
    got, mats = call(torch, b, case[0], x, y, w, cuts, ev, device=device, **kw)
    return b, got, mats


def test_the_audited_settings_reach_gamma_and_the_child_minimum():
    """From the restatement alone, as tests/test_grow_quantile_audit_cpu.py asserts without a GPU."""
    got = {c: A.q_reaches(c) for c in A.Q_CASES}
    for setting, kw in A.Q_SETTINGS.items():
        if kw.get("gamma", 0.0) > 0:
            assert any(got[c]["mixed"] for c in A.Q_CASES if c[3] == setting), (setting, "a level with a split beside a node that gamma closed")
        if kw.get("min_child_weight", 0.0) > 0:
            assert any(got[c]["moved"] for c in A.Q_CASES if c[3] == setting), (setting, "a split that min_child_weight moved")
    for c in A.Q_CASES:
        assert all(v >= 1 for v in got[c]["weightless"]) and (c[0] != "sampled" or all(v >= 1 for v in got[c]["out_of_bag"])), c


@pytest.mark.parametrize("case", A.Q_CASES, ids=A.q_id)
def test_off_default_quantile_trees_against_the_restatement(torch_cuda, tmp_path, case):
    x, y, w, cuts, ev, want = A.q_restated(case)
    assert want["rounds_run"] == 2 and len(want["trees"]) == 2
    b, got, mats = q_call(torch_cuda, case, x, y, w, cuts, ev, case[1] == "device")
    same_result(got, want, A.q_id(case))
    same_new_trees(held(b, tmp_path)[0], want["trees"], 0, A.q_id(case))
    assert saved(b, tmp_path) == expected_images(tmp_path, want["trees"]), "the bytes of a model that holds the restated trees"
    d = capi.DMatrix(x, missing=NAN)
    assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want["pred"])), (A.q_id(case), "XGBoosterPredict")
    done(b, mats + [d])


@pytest.mark.parametrize("case", A.Q_CASES, ids=A.q_id)
def test_the_quantile_trees_the_library_grew_pass_the_audit(torch_cuda, tmp_path, case):
    """In the form the comparison above does not take.  The audit knows the rows, the labels and the library's trees, not the
    restatement: a round's pairs and residuals come from the margins of the library's earlier trees walked on the host, and a
    leaf's rows from the audit's own walk of the library's tree over the binned rows."""
    x, y, w, cuts, ev, want = A.q_restated(case)
    b, got, mats = q_call(torch_cuda, case, x, y, w, cuts, ev, case[1] == "host")
    trees, _ = held(b, tmp_path)
    done(b, mats)
    assert got["nodes_added"] == sum(len(t["left"]) for t in trees) and len(trees) == A.ROUNDS
    audits = A.q_audits(case, x, y, w, cuts, trees)
    in_bags = [P.bag(A.q_hyper(case).get("seed", 0), r, len(y), A.q_hyper(case).get("subsample", 1.0)) for r in range(len(trees))]
    for r, (a, pred) in enumerate(audits):
        assert a.leaf_rule is None and a.violations() == [], (A.q_id(case), "tree", r)
        assert A.quantile_leaf_violations(a, pred, y, case[2]) == [], (A.q_id(case), "tree", r)
        leaves = [p for p in a.order if trees[r]["left"][p] < 0]
        assert any(np.any(in_bags[r][a.rows[p]] & (w[a.rows[p]] == 0)) for p in leaves), "a leaf that holds a row of weight 0"
        if case[0] == "sampled":
            assert any(not np.all(in_bags[r][a.rows[p]]) for p in leaves), "a leaf that holds a row out of the bag"
    records, pinned = (sum(a.stats[k] for a, _ in audits) for k in ("records", "pinned"))
    assert pinned >= 0.95 * records, "the bounds pin nearly every float32 record to one value"
    assert sum(A.decided(a) for a, _ in audits) >= 10, "splits at which a wrong choice would be reported"
    same_new_trees(trees, want["trees"], 0, A.q_id(case))


# ---- 12. a tie is no improvement ----

def test_a_tie_of_the_pinball_sums_is_no_improvement(torch_cuda, tmp_path):
    x, y, w, cuts, ev, want = Q.tie_case()
    assert len(want["all_trees"]) == 1 and all(len(t["left"]) == 1 and helpers.bits(t["value"])[0] == 0 for t in want["all_trees"]), "one leaf of +0.0"
    assert want["eval_sums"][1] == want["eval_sums"][0] > 1 << 64, "a tie of integers of three parts"
    assert (want["rounds_run"], want["best_round"], want["nodes_added"], want["trees"]) == (1, 0, 0, [])
    params = (("ohx_objective", "quantile"), ("ohx_quantile_alpha", "0.5"), ("ohx_eval_metric", "quantile"))
    for device in (False, True):
        b = booster(params, nfeat=3)
        before = saved(b, tmp_path)
        got, mats = call(torch_cuda, b, "weighted", x, y, w, cuts, ev, device=device, rounds=3, max_depth=6, eta=0.125, reg_lambda=1.0,
                         gamma=1e6, min_child_weight=0.0, patience=1)
        same_result(got, want, "a tie under patience 1")
        assert saved(b, tmp_path) == before and held(b, tmp_path)[0] == [], "nothing is appended"
        done(b, mats)
