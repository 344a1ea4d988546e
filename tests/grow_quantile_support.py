"""Shared by the tests of quantile boosting ("ohx_objective" = quantile, "ohx_quantile_alpha", "ohx_eval_metric" = quantile): a
restatement in numpy and Python integers of the text of include/ohxgb.h - the pair, the leaf as the lower weighted
alpha-quantile of the leaf's residuals, the pinball sums - and of a whole boost call assembled from the other restatements'
pieces (cuts, bins, histograms, split choice, bag, held-out walk, stop rule).  Nothing here calls the code under test.

The leaf is found by sorting: the keys of the rows that count are sorted, their hq cumulated as Python ints, and k* is the
first key at which alpha_q * W <= 2^24 * C(k) holds - no radix, no passes, no bins."""
import functools

import numpy as np

from tests import grow_eval_support as E
from tests import grow_objective_support as O
from tests import grow_reg_support as RG
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests import grow_weighted_support as W
from tests import refit_support as R

F32 = np.float32
MIN_ALPHA, MAX_ALPHA = 2.0 ** -10, 1.0 - 2.0 ** -10
ALPHAS = (2.0 ** -10, 0.05, 0.5, 0.95, 1.0 - 2.0 ** -10)
ONE = 1 << 24
BASE = O.BASE


def check_alpha(alpha):
    a = F32(alpha)
    if not (np.isfinite(a) and a >= F32(MIN_ALPHA) and a <= F32(MAX_ALPHA)):
        raise ValueError("ohx_quantile_alpha: not finite, < 2^-10 or > 1 - 2^-10")
    return a


def alpha_q(alpha):
    """(uint32) rint(alpha * 2^24) of the float32 alpha, a Python int."""
    scaled = check_alpha(alpha) * R.SCALE
    assert isinstance(scaled, F32)
    q = int(np.rint(scaled))
    assert (1 << 14) <= q <= ONE - (1 << 14)
    return q


# ---- the pair ----

def pairs(alpha, pred, y, w=None):
    """The header's quantile pair of every row -> (q int64 [n], hq uint64 [n]); raises as grow_objective_support.pairs."""
    a = check_alpha(alpha)
    z = W.residuals(pred, y)
    wt = np.ones(len(z), F32) if w is None else W.check_weights(w, "weight")
    g = np.where(z >= F32(0.0), F32(1.0) - a, -a)
    assert g.dtype == F32
    with np.errstate(under="ignore"):
        q = W.grad_fixed(g, wt)
        hq = W.hess_fixed(wt)          # h = 1.0f: hw = w
    return q, hq


# ---- the leaf ----

def keys(r):
    """key(bits(r)) of the float32 residuals r: -0.0f as +0.0f, negative floats flipped whole, the others get their sign bit."""
    u = np.ascontiguousarray(r, dtype=F32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u >> 31 != 0, u ^ np.uint32(0xFFFFFFFF), u ^ np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = int(k)
    u = k ^ (0x80000000 if k >> 31 else 0xFFFFFFFF)
    return np.asarray([u], np.uint32).view(F32)[0]


def leaf_key(k, hq, aq):
    """k* of one leaf from the keys and hessians of its rows, or None where the rows that count hold no weight."""
    k, hq = np.asarray(k, np.uint32), np.asarray(hq, np.uint64)
    keep = hq > 0
    k, hq = k[keep], hq[keep]
    Wp = sum(int(h) for h in hq)
    if Wp == 0:
        return None
    order = np.argsort(k, kind="stable")
    C = 0
    ks, hs = k[order], hq[order]
    i = 0
    while i < len(ks):
        j = i
        while j < len(ks) and ks[j] == ks[i]:
            C += int(hs[j])
            j += 1
        if aq * Wp <= ONE * C:
            return int(ks[i])
        i = j
    raise AssertionError("alpha_q <= 2^24: the rule holds at the largest key")


def leaf_key_fast(k, hq, aq):
    """leaf_key for many rows: the cumulated sums as Python ints over a sorted array (the same rule)."""
    k, hq = np.asarray(k, np.uint32), np.asarray(hq, np.uint64)
    keep = hq > 0
    k, hq = k[keep], hq[keep]
    if len(k) == 0:
        return None
    order = np.argsort(k, kind="stable")
    ks = k[order]
    cum = np.cumsum(hq[order].astype(object))
    Wp = int(cum[-1])
    last = np.flatnonzero(np.append(ks[1:] != ks[:-1], True))      # the last row of every distinct key: C(k)
    for i in last:
        if aq * Wp <= ONE * int(cum[i]):
            return int(ks[i])
    raise AssertionError("alpha_q <= 2^24: the rule holds at the largest key")


def leaf_value(kstar, eta):
    v = unkey(kstar) * F32(eta)
    assert isinstance(v, F32)
    return v


def covers(k, hq, aq, kstar):
    """The property itself, from nothing but comparisons: 2^24 C(k*) >= alpha_q W and 2^24 C(k* - 1) < alpha_q W."""
    k, hq = np.asarray(k, np.uint32), np.asarray(hq, np.uint64).astype(object)
    Wp = int(hq.sum()) if len(hq) else 0
    upto = int(hq[k <= np.uint32(kstar)].sum()) if np.any(k <= np.uint32(kstar)) else 0
    below = int(hq[k < np.uint32(kstar)].sum()) if np.any(k < np.uint32(kstar)) else 0
    return ONE * upto >= aq * Wp and ONE * below < aq * Wp


def set_leaves(t, pos, hb, pred, y, alpha, eta):
    """The header's leaf update of the tree t in place: pos the node of every row after the last level, hb the hessians that
    count (0 out of the bag), pred the margin at the start of the round.  -> {leaf node: k*} of the leaves that were set."""
    aq = alpha_q(alpha)
    r = np.asarray(y, F32) - np.asarray(pred, F32)
    assert r.dtype == F32
    k = keys(r)
    out = {}
    for p in np.flatnonzero(t["left"] < 0):
        rows = np.flatnonzero(pos == p)
        ks = leaf_key_fast(k[rows], hb[rows], aq)
        if ks is None:
            continue                    # W_p == 0: the record stays
        t["value"][p] = leaf_value(ks, eta)
        out[int(p)] = ks
    return out


# ---- the metric ----

def pinball_terms(alpha, z):
    """sq of the header for the sound float32 residuals z = pred - y -> an object array of Python ints."""
    aq = alpha_q(alpha)
    z = np.asarray(z, dtype=F32)
    scaled = z * R.SCALE
    assert scaled.dtype == F32
    m = np.abs(np.rint(scaled).astype(np.int64)).astype(object)
    f = np.where(z < F32(0.0), aq, ONE - aq).astype(object)
    return m * f


def metric_sum(metric, slope, alpha, z, hq):
    if metric != "quantile":
        return RG.metric_sum(metric, slope, z, hq)
    sq = pinball_terms(alpha, z)
    return int((np.asarray(hq).astype(object) * sq).sum()) if len(sq) else 0


def metric_value(metric, S, Wsum):
    if metric != "quantile":
        return RG.metric_value(metric, S, Wsum)
    return (float(S) * 2.0 ** -72) / (float(Wsum) * 2.0 ** -24)


# ---- a boost call ----

def boost(objective, alpha, pred, x, missing, y, w, cuts, num_feature, eval_set=None, eval_pred=None, rounds=1, patience=0,
          max_depth=6, eta=0.3, lam=1.0, gamma=0.0, min_child_weight=1.0, subsample=1.0, colsample_bytree=1.0, seed=0, tree0=0,
          metric="rmse", slope=1.0):
    """grow_objective_support.boost with the objective "quantile" beside its two (then `alpha` is not read by the pair) and
    any metric.  -> its dict, with "leaf_keys": per tree {leaf: k*}.  train_rmse / eval_rmse hold the metric's values."""
    assert max_depth <= 8 or objective != "quantile"
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
        eval_sums = [metric_sum(metric, slope, alpha, eg0, ehq)]
    else:
        assert patience == 0
        eval_sums, eW, epred = None, None, None
    train_sums = [metric_sum(metric, slope, alpha, g0, mq)]
    trees, preds, epreds, leaf_keys, poss, hbs = [], [pred.copy()], [epred.copy() if epred is not None else None], [], [], []
    run, best = rounds, 0
    for r in range(rounds):
        q, hq = pairs(alpha, pred, y, wt) if objective == "quantile" else O.pairs(objective, slope, pred, y, wt)
        in_bag = P.bag(seed, tree0 + r, n, subsample)
        kept = P.features(seed, tree0 + r, num_feature, colsample_bytree)
        qb, hb = np.where(in_bag, q, 0).astype(np.int64), np.where(in_bag, hq, 0).astype(np.uint64)
        if int(hb.astype(object).sum()) == 0:
            if objective == "pseudohuber":
                raise ValueError("hessian: the root of round %d holds no hessian" % (r + 1))
            if subsample != 1.0 or colsample_bytree != 1.0:
                raise ValueError("bag: the bag of round %d holds no weight" % (r + 1))
        t, pos = W.grow_tree(bins, qb, hb, P.emptied_cuts(cuts, num_feature, kept), max_depth, eta, lam, gamma, min_child_weight)
        leaf_keys.append(set_leaves(t, pos, hb, pred, y, alpha, eta) if objective == "quantile" else {})
        poss.append(pos)
        hbs.append(hb)
        pred = pred + t["value"][pos]
        assert pred.dtype == F32
        trees.append(t)
        preds.append(pred.copy())
        train_sums.append(metric_sum(metric, slope, alpha, W.residuals(pred, y), mq))
        if eval_set is not None:
            epred = epred + E.walk(t, ex, emissing)
            assert epred.dtype == F32
            epreds.append(epred.copy())
            eval_sums.append(metric_sum(metric, slope, alpha, W.residuals(epred, ey, "eval label"), ehq))
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
            "pred": preds[keep], "eval_pred": epreds[keep] if eval_set is not None else None, "preds": preds,
            "leaf_keys": leaf_keys, "pos": poss, "hessians": hbs}


def inputs(n, seed, nfeat=3, bins=32, held_out=0, missing=float("nan")):
    """grow_objective_support.inputs with the missing value of choice (-999: the NaNs become it) and, for small n, cuts that
    the rows at hand can make."""
    x, y, w, cuts, ev = O.inputs(n, seed, nfeat, bins, held_out)
    if not np.isnan(missing):
        x = np.where(np.isnan(x), F32(missing), x).astype(F32)
        cuts = G.quantile_cuts(x, missing, bins)
        if ev is not None:
            ev = (np.where(np.isnan(ev[0]), F32(missing), ev[0]).astype(F32), missing, ev[2], ev[3])
    return x, y, w, cuts, ev


@functools.lru_cache(maxsize=None)
def restated(objective, alpha, n, seed, max_depth, bins=32, nfeat=3, rounds=2, held_out=0, patience=0, subsample=1.0,
             colsample=1.0, draw_seed=0, lam=1.0, mcw=0.0, weighted=True, eta=0.125, gamma=0.0, metric="rmse", slope=1.0,
             missing=float("nan")):
    """One restated case, computed once and shared (the result is not to be changed).  -> (x, y, w, cuts, ev, the dict)."""
    x, y, w, cuts, ev = inputs(n, seed, nfeat, bins, held_out, missing)
    if not weighted:
        w = None
        ev = (ev[0], ev[1], ev[2], None) if ev is not None else None
    want = boost(objective, alpha, np.full(n, BASE, F32), x, missing, y, w, cuts, nfeat, eval_set=ev,
                 eval_pred=np.full(held_out, BASE, F32) if held_out else None, rounds=rounds, patience=patience,
                 max_depth=max_depth, eta=eta, lam=lam, gamma=gamma, min_child_weight=mcw, subsample=subsample,
                 colsample_bytree=colsample, seed=draw_seed, metric=metric, slope=slope)
    return x, y, w, cuts, ev, want


@functools.lru_cache(maxsize=None)
def tie_case(n=1300, held_out=400, seed=3330, alpha=0.5, rounds=3):
    """A call whose held-out pinball sum does not move: four labels in five equal the base, so the root's quantile is the
    residual +0.0, and gamma is large enough that no round splits.  Every tree is one leaf of value +0.0, the margins stay
    where they were, and the sum after round 1 ties with the sum before it: under patience = 1 that is no improvement.
    -> (x, y, w, cuts, ev, the dict of boost; not to be changed)."""
    x, y, w, cuts, ev = inputs(n, seed, 3, 32, held_out)
    at_base = np.random.default_rng(seed + 1).random(n) < 0.8
    y = np.where(at_base, F32(BASE), y).astype(F32)
    want = boost("quantile", alpha, np.full(n, BASE, F32), x, float("nan"), y, w, cuts, 3, eval_set=ev, eval_pred=np.full(held_out, BASE, F32),
                 rounds=rounds, patience=1, max_depth=6, eta=0.125, lam=1.0, gamma=1e6, min_child_weight=0.0, metric="quantile")
    return x, y, w, cuts, ev, want


# ---- crafted leaves: the edges of the select ----

BELOW_256 = np.nextafter(F32(256.0), F32(0.0))


def crafted_leaves():
    """[(name, residuals float32, weights float32)]: each the rows of one leaf.  Every |r| < 256 and 0 <= w < 256."""
    rng = np.random.default_rng(3200)
    low = (np.uint32(0x3F800000) + np.arange(256, dtype=np.uint32)).view(F32)
    high = np.asarray([s * 2.0 ** e for e in (-120, -60, -20, 0, 6) for s in (-1.0, 1.0)], F32)
    edge_w = np.asarray([0.0, 2.0 ** -24, BELOW_256], F32)
    return [
        ("one row", np.asarray([1.5], F32), np.ones(1, F32)),
        ("all equal", np.full(5, 2.0, F32), np.asarray([1.0, 2.0, 0.5, 0.0, 2.0 ** -24], F32)),
        ("the lowest 8 key bits", low, np.ones(256, F32)),
        ("the highest 8 key bits", high, np.ones(len(high), F32)),
        ("+0.0 against -0.0", np.asarray([0.0, -0.0, 0.0, -0.0, -1.0, 1.0], F32), np.ones(6, F32)),
        ("both signs", np.asarray([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0, -2.0 ** -149, 2.0 ** -149], F32), np.ones(8, F32)),
        ("weights 0, 2^-24 and just below 256", rng.standard_normal(12).astype(F32), np.tile(edge_w, 4)),
        ("every row weighs 0", np.asarray([1.0, 2.0, 3.0], F32), np.zeros(3, F32)),
    ]
