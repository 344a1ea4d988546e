"""Shared by the tests of "ohx_reg_alpha", "ohx_max_delta_step" and "ohx_eval_metric": a restatement in numpy and Python
floats and integers of the regularised gain and leaf and of the three metrics, written from the text of include/ohxgb.h
alone, and of a boost call that grows its trees with them.  Nothing here calls the code under test.

The policy is Python floats (IEEE doubles) in the header's order, one rounding an operation; base_weight is np.float32 of
the double and the leaf one np.float32 multiply.  A tree is grow_weighted_support.grow_tree itself, run over a copy of that
module's globals in which `gain` and `solve` are the regularised ones (the module is not touched): the candidates, their
order, the ties, min_child_weight and the node numbering are therefore the weighted call's by construction.  A row's term
of a metric is np.float32 operations (numpy fuses nothing; its division and square root are IEEE, and it keeps
denormals); S and W are Python ints.  The pairs, the bag, the lists, the held-out walk and the stop rule are those of the
other restatements."""
import functools
import math
import types

import numpy as np

from tests import grow_eval_support as E
from tests import grow_objective_support as O
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests import grow_weighted_support as W
from tests import refit_support as R

METRICS = ("rmse", "mae", "pseudohuber")
F32 = np.float32
BASE = O.BASE


def check_reg(v, name):
    v = F32(v)
    if not (np.isfinite(v) and v >= 0):
        raise ValueError(f"{name}: not finite or negative")
    return float(v)


# ---- the policy ----

def threshold_l1(Gd, alpha):
    return Gd - alpha if Gd > alpha else (Gd + alpha if Gd < -alpha else 0.0)


def weight(Gd, D, alpha, m):
    """w of the header: (-T) / D, clipped to +-m where m > 0.  D == 0 (no hessian and lambda 0) divides as IEEE does."""
    T = threshold_l1(Gd, alpha)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = float(np.float64(-T) / np.float64(D))
    if m > 0 and abs(w) > m:
        w = math.copysign(m, w)
    return w


def gain(Gs, H, lam, alpha, m):
    Gd = float(int(Gs)) * 2.0 ** -24
    D = W.hess(H) + float(F32(lam))
    alpha, m = float(F32(alpha)), float(F32(m))
    if m == 0:
        T = threshold_l1(Gd, alpha)
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(np.float64(T * T) / np.float64(D))
    w = weight(Gd, D, alpha, m)
    return -((2.0 * Gd) * w + (D * w) * w) - (2.0 * alpha) * abs(w)


def solve(Gs, H, eta, lam, alpha, m):
    """(leaf, base_weight, sum_hess) float32."""
    Gd = float(int(Gs)) * 2.0 ** -24
    w = F32(weight(Gd, W.hess(H) + float(F32(lam)), float(F32(alpha)), float(F32(m))))
    leaf = w * F32(eta)
    assert leaf.dtype == F32
    return leaf, w, F32(W.hess(H))


def tree_grower(alpha, m, seen=None):
    """grow_weighted_support.grow_tree with the regularised gain and leaf.  seen: a list that receives (G, H, base_weight)
    of every node of every tree grown, in node order."""
    g = dict(W.__dict__)

    def reg_solve(Gs, H, eta, lam):
        out = solve(Gs, H, eta, lam, alpha, m)
        if seen is not None:
            seen.append((int(Gs), int(H), out[1]))
        return out

    g["gain"] = lambda Gs, H, lam: gain(Gs, H, lam, alpha, m)
    g["solve"] = reg_solve
    g["best_split"] = types.FunctionType(W.best_split.__code__, g, "best_split")
    return types.FunctionType(W.grow_tree.__code__, g, "grow_tree")


def binding(seen, m):
    """(clipped, zeroed, neither) over the nodes `seen`: |base_weight| == m; G != 0 and base_weight == 0; the rest."""
    clipped = sum(1 for _, _, w in seen if m > 0 and abs(w) == F32(m))
    zeroed = sum(1 for Gs, _, w in seen if Gs != 0 and w == 0)
    return clipped, zeroed, len(seen) - clipped - zeroed


# ---- the metrics ----

def metric_terms(metric, slope, z):
    """sq of the header for the sound float32 residuals z -> an object array of Python ints."""
    assert metric in METRICS
    z = np.asarray(z, dtype=F32)
    if metric == "pseudohuber":
        d = O.check_slope(slope)
        with np.errstate(under="ignore"):
            d2 = d * d
            z2 = z * z
            s = np.sqrt(F32(1.0) + z2 / d2)
            mf = z2 / (F32(1.0) + s)
            scaled = mf * R.SCALE
        assert all(v.dtype == F32 for v in (z2, s, mf, scaled)) and isinstance(d2, F32)
        return np.rint(scaled).astype(np.uint64).astype(object)
    scaled = z * R.SCALE
    assert scaled.dtype == F32
    e = np.abs(np.rint(scaled).astype(np.int64)).astype(object)
    return e * e if metric == "rmse" else e


def metric_sum(metric, slope, z, hq):
    """S = sum hq * sq as a Python int."""
    sq = metric_terms(metric, slope, z)
    return int((np.asarray(hq).astype(object) * sq).sum()) if len(sq) else 0


def metric_value(metric, S, Wsum):
    if metric == "rmse":
        return W.rmse(S, Wsum)
    return (float(S) * 2.0 ** -48) / (float(Wsum) * 2.0 ** -24)


# ---- a boost call ----

def boost(objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, eval_set=None, eval_pred=None, rounds=1,
          patience=0, max_depth=6, eta=0.3, lam=1.0, gamma=0.0, min_child_weight=1.0, subsample=1.0, colsample_bytree=1.0, seed=0,
          tree0=0):
    """grow_objective_support.boost with the regularised policy and the metric `metric` (delta is `slope` whatever the
    objective).  -> its dict, with "seen": per tree the (G, H, base_weight) of its nodes.  train_rmse / eval_rmse hold the
    metric's values, as the call's arrays do."""
    alpha, m = check_reg(alpha, "ohx_reg_alpha"), check_reg(m, "ohx_max_delta_step")
    pred = np.asarray(pred, dtype=F32).copy()
    y = np.asarray(y, dtype=F32)
    n = len(y)
    P.threshold(subsample)
    P.num_selected(num_feature, colsample_bytree)
    wt = np.ones(n, F32) if w is None else np.asarray(w, dtype=F32)
    bins = G.bin_rows(x, missing, cuts, num_feature)
    g0 = W.residuals(pred, y)
    wt = W.check_weights(wt, "weight")
    mq = W.hess_fixed(wt)
    Wsum = int(mq.astype(object).sum())
    if eval_set is not None:
        ex, emissing, ey, ew = (tuple(eval_set) + (None,))[:4]
        ey = np.asarray(ey, dtype=F32)
        ewt = np.ones(len(ey), F32) if ew is None else np.asarray(ew, dtype=F32)
        epred = np.asarray(eval_pred, dtype=F32).copy()
        eg0 = W.residuals(epred, ey, "eval label")
        ewt = W.check_weights(ewt, "eval weight")
        ehq = W.hess_fixed(ewt)
        eW = int(ehq.astype(object).sum())
        eval_sums = [metric_sum(metric, slope, eg0, ehq)]
    else:
        assert patience == 0
        eval_sums, eW, epred = None, None, None
    train_sums = [metric_sum(metric, slope, g0, mq)]
    trees, preds, epreds, seen = [], [pred.copy()], [epred.copy() if epred is not None else None], []
    run, best = rounds, 0
    for r in range(rounds):
        q, hq = O.pairs(objective, slope, pred, y, wt)
        in_bag = P.bag(seed, tree0 + r, n, subsample)
        kept = P.features(seed, tree0 + r, num_feature, colsample_bytree)
        qb, hb = np.where(in_bag, q, 0).astype(np.int64), np.where(in_bag, hq, 0).astype(np.uint64)
        if int(hb.astype(object).sum()) == 0:
            if objective == "pseudohuber":
                raise ValueError("hessian: the root of round %d holds no hessian" % (r + 1))
            if subsample != 1.0 or colsample_bytree != 1.0:
                raise ValueError("bag: the bag of round %d holds no weight" % (r + 1))
        nodes = []
        t, pos = tree_grower(alpha, m, nodes)(bins, qb, hb, P.emptied_cuts(cuts, num_feature, kept), max_depth, eta, lam, gamma,
                                              min_child_weight)
        pred = pred + t["value"][pos]
        assert pred.dtype == F32
        trees.append(t)
        seen.append(nodes)
        preds.append(pred.copy())
        train_sums.append(metric_sum(metric, slope, W.residuals(pred, y), mq))
        if eval_set is not None:
            epred = epred + E.walk(t, ex, emissing)
            assert epred.dtype == F32
            epreds.append(epred.copy())
            eval_sums.append(metric_sum(metric, slope, W.residuals(epred, ey, "eval label"), ehq))
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
            "eval_W": eW, "train_rmse": [metric_value(metric, s, Wsum) for s in train_sums],
            "eval_rmse": [metric_value(metric, s, eW) for s in eval_sums] if eval_sums is not None else None,
            "rounds_run": run, "best_round": best, "nodes_added": sum(len(t["left"]) for t in kept_trees),
            "pred": preds[keep], "eval_pred": epreds[keep] if eval_set is not None else None, "preds": preds, "seen": seen}


@functools.lru_cache(maxsize=None)
def restated(objective, slope, alpha, m, metric, n, seed, max_depth, bins=64, nfeat=3, rounds=2, held_out=0, patience=0,
             subsample=1.0, colsample=1.0, draw_seed=0, lam=1.0, mcw=0.0, weighted=True, eta=0.125, gamma=0.0):
    """One restated case on grow_objective_support.inputs, computed once and shared (the result is not to be changed).
    -> (x, y, w, cuts, ev, the dict of boost)."""
    x, y, w, cuts, ev = O.inputs(n, seed, nfeat, bins, held_out)
    if not weighted:
        w = None
        ev = (ev[0], ev[1], ev[2], None) if ev is not None else None
    want = boost(objective, slope, alpha, m, metric, np.full(n, BASE, F32), x, float("nan"), y, w, cuts, nfeat, eval_set=ev,
                 eval_pred=np.full(held_out, BASE, F32) if held_out else None, rounds=rounds, patience=patience,
                 max_depth=max_depth, eta=eta, lam=lam, gamma=gamma, min_child_weight=mcw, subsample=subsample,
                 colsample_bytree=colsample, seed=draw_seed)
    return x, y, w, cuts, ev, want
