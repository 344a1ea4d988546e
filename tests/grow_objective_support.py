"""Shared by the tests of the boosting objectives ("ohx_objective"): a restatement in numpy of the (gradient, hessian) pair
of include/ohxgb.h, written from the header's text alone, and of a boost call that grows its trees from those pairs.
Nothing here calls the code under test.

Every operation of the pair is an np.float32 operation, which rounds once (numpy fuses nothing; its float32 division and
square root are IEEE); q and hq are np.rint of the float32 product with 2^24, which is exact.  A tree is
grow_weighted_support.grow_tree given q and hq (zeroed out of the bag, the cuts of unselected features emptied, as
grow_sampled_support does); the metric is grow_weighted_support's, weighted by rint(w * 2^24) whatever the objective; the
held-out walk and the stop rule are those of the other restatements."""
import functools

import numpy as np

from tests import grow_eval_support as E
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests import grow_weighted_support as W
from tests import refit_support as R

OBJECTIVES = ("squarederror", "pseudohuber")
MIN_SLOPE, MAX_SLOPE = 2.0 ** -10, 256.0
F32 = np.float32


def check_slope(slope):
    s = F32(slope)
    if not (np.isfinite(s) and s >= F32(MIN_SLOPE) and s <= F32(MAX_SLOPE)):
        raise ValueError("ohx_huber_slope: not finite, < 2^-10 or > 256")
    return s


def pair_floats(objective, slope, z):
    """(g, h) float32 of the residuals z (float32, sound), before the weight."""
    assert objective in OBJECTIVES
    z = np.asarray(z, dtype=F32)
    if objective == "squarederror":
        return z, np.ones_like(z)
    d = check_slope(slope)
    with np.errstate(under="ignore"):
        d2 = d * d
        z2 = z * z
        s = np.sqrt(F32(1.0) + z2 / d2)
        g = z / s
        c = d2 + z2
        h = d2 / (c * s)
    assert all(v.dtype == F32 for v in (z2, s, g, c, h)) and isinstance(d2, F32)
    return g, h


def pairs(objective, slope, pred, y, w=None):
    """The header's pair of every row -> (q int64 [n], hq uint64 [n]).  Raises ValueError("label ..") or ("weight ..") where a
    row is refused: the residual before the weight, then the weight, then the weighted gradient."""
    z = W.residuals(pred, y)
    wt = np.ones(len(z), F32) if w is None else W.check_weights(w, "weight")
    g, h = pair_floats(objective, slope, z)
    with np.errstate(under="ignore"):
        q = W.grad_fixed(g, wt)       # gw = g * w in float32; "label" at |gw| >= 256; rint(gw * 2^24)
        hw = h * wt
        assert hw.dtype == F32
        scaled = hw * R.SCALE
    assert scaled.dtype == F32
    hq = np.rint(scaled).astype(np.uint64)
    assert np.all(hq < (1 << 32))
    return q, hq


def boost(objective, slope, pred, x, missing, y, w, cuts, num_feature, eval_set=None, eval_pred=None, rounds=1, patience=0,
          max_depth=6, eta=0.3, lam=1.0, gamma=0.0, min_child_weight=1.0, subsample=1.0, colsample_bytree=1.0, seed=0, tree0=0):
    """grow_sampled_support.boost_sampled (at (1, 1): grow_weighted_support.boost_weighted; max_depth up to 18: the Deep
    calls) with the pairs of `objective`.  -> its dict.  Raises ValueError with "label", "eval label", "weight",
    "eval weight", "bag", "hessian" or "sum to 0" where the call is refused."""
    pred = np.asarray(pred, dtype=F32).copy()
    y = np.asarray(y, dtype=F32)
    n = len(y)
    P.threshold(subsample)
    P.num_selected(num_feature, colsample_bytree)
    wt = np.ones(n, F32) if w is None else np.asarray(w, dtype=F32)
    bins = G.bin_rows(x, missing, cuts, num_feature)
    g0 = W.residuals(pred, y)
    wt = W.check_weights(wt, "weight")
    mq = W.hess_fixed(wt)                                # the metric's weights: rint(w * 2^24), constant over the rounds
    if eval_set is not None:
        ex, emissing, ey, ew = (tuple(eval_set) + (None,))[:4]
        ey = np.asarray(ey, dtype=F32)
        ewt = np.ones(len(ey), F32) if ew is None else np.asarray(ew, dtype=F32)
        epred = np.asarray(eval_pred, dtype=F32).copy()
        eg0 = W.residuals(epred, ey, "eval label")
        ewt = W.check_weights(ewt, "eval weight")
        ehq = W.hess_fixed(ewt)
        eS0, eW = W.weighted_sum(eg0, ehq)
        eval_sums = [eS0]
    else:
        assert patience == 0
        eval_sums, eW, epred = None, None, None
    S0, Wsum = W.weighted_sum(g0, mq)
    train_sums = [S0]
    trees, preds, epreds, bags, feats, hqs = [], [pred.copy()], [epred.copy() if epred is not None else None], [], [], []
    run, best = rounds, 0
    for r in range(rounds):
        q, hq = pairs(objective, slope, pred, y, wt)     # every row, in or out of the bag
        in_bag = P.bag(seed, tree0 + r, n, subsample)
        kept = P.features(seed, tree0 + r, num_feature, colsample_bytree)
        qb, hb = np.where(in_bag, q, 0).astype(np.int64), np.where(in_bag, hq, 0).astype(np.uint64)
        if int(hb.astype(object).sum()) == 0:
            if objective == "pseudohuber":
                raise ValueError("hessian: the root of round %d holds no hessian" % (r + 1))
            if subsample != 1.0 or colsample_bytree != 1.0:
                raise ValueError("bag: the bag of round %d holds no weight" % (r + 1))
        t, pos = W.grow_tree(bins, qb, hb, P.emptied_cuts(cuts, num_feature, kept), max_depth, eta, lam, gamma, min_child_weight)
        pred = pred + t["value"][pos]
        assert pred.dtype == F32
        trees.append(t)
        bags.append(in_bag)
        feats.append(kept)
        hqs.append(hq)
        preds.append(pred.copy())
        train_sums.append(W.weighted_sum(W.residuals(pred, y), mq)[0])
        if eval_set is not None:
            epred = epred + E.walk(t, ex, emissing)
            assert epred.dtype == F32
            epreds.append(epred.copy())
            eval_sums.append(W.weighted_sum(W.residuals(epred, ey, "eval label"), ehq)[0])
            if eval_sums[r + 1] < eval_sums[best]:
                best = r + 1
            if patience >= 1 and (r + 1) - best >= patience:
                run = r + 1
                break
    if Wsum == 0:
        raise ValueError("the weights sum to 0")
    if eval_set is not None and eW == 0:
        raise ValueError("the eval weights sum to 0")
    if eval_set is None:
        best = run
    keep = best if patience >= 1 else rounds
    kept_trees = trees[:keep]
    return {"trees": kept_trees, "all_trees": trees, "train_sums": train_sums, "eval_sums": eval_sums, "train_W": Wsum,
            "eval_W": eW, "train_rmse": [W.rmse(s, Wsum) for s in train_sums],
            "eval_rmse": [W.rmse(s, eW) for s in eval_sums] if eval_sums is not None else None,
            "rounds_run": run, "best_round": best, "nodes_added": sum(len(t["left"]) for t in kept_trees),
            "pred": preds[keep], "eval_pred": epreds[keep] if eval_set is not None else None, "preds": preds,
            "bags": bags, "features": feats, "hessians": hqs}


BASE = 0.5          # the margin of grow_support.empty_model


def inputs(n, seed, nfeat=3, bins=64, held_out=0):
    """-> (x float32 [n][nfeat] standard normal with 5 % missing, y = sin(3 x0) + 0.3 noise with one label in twelve thrown
    out by up to +-40, w from {0, 0.5, .., 2}, the quantile cuts, ev = (rows, NaN, labels, weights) of the same kind, or
    None)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, nfeat)).astype(F32)
    x0 = x[:, 0].copy()
    x[rng.random((n, nfeat)) < 0.05] = np.nan
    y = (np.sin(3.0 * x0) + 0.3 * rng.standard_normal(n)).astype(F32)
    wild = rng.random(n) < 1.0 / 12.0
    y[wild] += (rng.uniform(-40.0, 40.0, n).astype(F32))[wild]
    w = rng.choice(np.arange(0.0, 2.5, 0.5).astype(F32), n)
    ev = None
    if held_out:
        ex = rng.standard_normal((held_out, nfeat)).astype(F32)
        ey = (np.sin(3.0 * ex[:, 0]) + 0.3 * rng.standard_normal(held_out)).astype(F32)
        ewild = rng.random(held_out) < 1.0 / 12.0
        ey[ewild] += (rng.uniform(-40.0, 40.0, held_out).astype(F32))[ewild]
        ex[rng.random((held_out, nfeat)) < 0.05] = np.nan
        ev = (ex, float("nan"), ey, rng.choice(np.arange(0.0, 2.5, 0.5).astype(F32), held_out))
    return x, y, w, G.quantile_cuts(x, float("nan"), bins), ev


def kind_kw(kind, deep_depth=11):
    """The hyper-parameters of a kind ("weighted", "sampled", "deep", "deep_sampled"), as the Python binding names them: the one
    point at which the GPU tests of the objectives, the regularisation and the constraints grow their trees
    (tests/grow_audit_support.py moves away from it)."""
    kw = dict(eta=0.125, reg_lambda=1.0, min_child_weight=0.0, max_depth=deep_depth if "deep" in kind else 6)
    if "sampled" in kind:
        kw.update(subsample=0.5, colsample_bytree=0.5, seed=11)
    return kw


@functools.lru_cache(maxsize=None)
def restated(objective, slope, n, seed, max_depth, bins=64, nfeat=3, rounds=2, held_out=0, patience=0, subsample=1.0,
             colsample=1.0, draw_seed=0, lam=1.0, mcw=0.0, weighted=True, eta=0.125, gamma=0.0):
    """One restated case on the common inputs, computed once and shared (the result is not to be changed).
    -> (x, y, w, cuts, ev, the dict of boost)."""
    x, y, w, cuts, ev = inputs(n, seed, nfeat, bins, held_out)
    if not weighted:
        w = None
        ev = (ev[0], ev[1], ev[2], None) if ev is not None else None
    want = boost(objective, slope, np.full(n, BASE, F32), x, float("nan"), y, w, cuts, nfeat, eval_set=ev,
                 eval_pred=np.full(held_out, BASE, F32) if held_out else None, rounds=rounds, patience=patience,
                 max_depth=max_depth, eta=eta, lam=lam, gamma=gamma, min_child_weight=mcw, subsample=subsample,
                 colsample_bytree=colsample, seed=draw_seed)
    return x, y, w, cuts, ev, want
