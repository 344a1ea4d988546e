"""Shared by the tests of boosting with row and column subsampling: a restatement of OHXBoosterBoostTreesSampled in
numpy, written from the text of include/ohxgb.h alone.  Nothing here calls the code under test.

The mix function, the tree keys, the bag and the feature keys are numpy uint64 arithmetic, which wraps; k_s is
np.rint of a float64 product and n_sel math.floor of one; the selected set is a sort of (c_f, f) pairs of Python ints.
A tree is grow_weighted_support.grow_tree given q and hq zeroed out of the bag and a cut pointer whose unselected
features are empty; everything else (residuals, weights, the sums over all rows, the held-out walk, the stop rule) is
grow_weighted_support's, over every row at its full weight."""
import math

import numpy as np

from tests import grow_eval_support as E
from tests import grow_support as G
from tests import grow_weighted_support as W

M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
GAMMA64 = np.uint64(0x9E3779B97F4A7C15)
ONE = 1 << 24


def mix(z):
    """z: uint64 scalar or array -> the same shape."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64).copy()
        z ^= z >> np.uint64(30)
        z *= M1
        z ^= z >> np.uint64(27)
        z *= M2
        z ^= z >> np.uint64(31)
    return z


def _u64(v):
    return np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


def row_key(seed, i):
    with np.errstate(over="ignore"):
        return mix(_u64(seed) + GAMMA64 * (np.uint64(2) * _u64(i) + np.uint64(1)))


def col_key(seed, i):
    with np.errstate(over="ignore"):
        return mix(_u64(seed) + GAMMA64 * (np.uint64(2) * _u64(i) + np.uint64(2)))


def threshold(subsample):
    """k_s = (uint32) rint((double)subsample * 2^24); raises where the call refuses the subsample."""
    s = np.float32(subsample)
    if not (np.isfinite(s) and s > 0 and s <= 1):
        raise ValueError("subsample: not finite, <= 0 or > 1")
    k = int(np.rint(np.float64(s) * np.float64(ONE)))
    if k == 0:
        raise ValueError("subsample: k_s == 0")
    return k


def bag(seed, i, nrow, subsample):
    """bool [nrow]: the rows in the bag of tree i."""
    k = threshold(subsample)
    if k == ONE:
        return np.ones(nrow, dtype=bool)
    with np.errstate(over="ignore"):
        draw = mix(row_key(seed, i) + np.arange(nrow, dtype=np.uint64))
    return (draw >> np.uint64(40)) < np.uint64(k)


def num_selected(F, colsample):
    c = np.float32(colsample)
    if not (np.isfinite(c) and c > 0 and c <= 1):
        raise ValueError("colsample_bytree: not finite, <= 0 or > 1")
    return max(1, int(math.floor(float(np.float64(c)) * F)))


def select(keys, n_sel):
    """The n_sel features smallest by (c_f, f), ascending in f.  keys: the c_f as Python ints."""
    order = sorted((int(c), f) for f, c in enumerate(keys))
    return sorted(f for _, f in order[:n_sel])


def features(seed, i, F, colsample):
    """The features tree i may split on, ascending."""
    n_sel = num_selected(F, colsample)
    if n_sel == F:
        return list(range(F))
    with np.errstate(over="ignore"):
        keys = mix(col_key(seed, i) + np.arange(F, dtype=np.uint64))
    return select(keys.tolist(), n_sel)


def emptied_cuts(cuts, num_feature, kept):
    """The cuts with an empty list for every feature not in `kept`: (cut_ptr uint64 [F + 1], cut_values float32)."""
    cut_ptr, cut_values = cuts
    ptr, vals = [0], []
    for f in range(num_feature):
        if f in kept:
            vals += list(cut_values[int(cut_ptr[f]):int(cut_ptr[f + 1])])
        ptr.append(len(vals))
    return np.asarray(ptr, dtype=np.uint64), np.asarray(vals, dtype=np.float32)


def boost_sampled(pred, x, missing, y, w, cuts, num_feature, eval_set=None, eval_pred=None, rounds=1, patience=0,
                  max_depth=6, eta=0.3, lam=1.0, gamma=0.0, min_child_weight=1.0, subsample=1.0, colsample_bytree=1.0,
                  seed=0, tree0=0):
    """grow_weighted_support.boost_weighted with the bag and the features of every round; tree0: the trees the forest
    holds when the call starts.  -> its dict, with `bags` and `features` per round grown.  Raises ValueError with "label",
    "eval label", "weight", "eval weight", "bag" or "sum to 0" where the call is refused."""
    pred = np.asarray(pred, dtype=np.float32).copy()
    y = np.asarray(y, dtype=np.float32)
    n = len(y)
    threshold(subsample)
    num_selected(num_feature, colsample_bytree)
    wt = np.ones(n, np.float32) if w is None else np.asarray(w, dtype=np.float32)
    bins = G.bin_rows(x, missing, cuts, num_feature)
    g0 = W.residuals(pred, y)
    wt = W.check_weights(wt, "weight")
    hq = W.hess_fixed(wt)
    if eval_set is not None:
        ex, emissing, ey, ew = (tuple(eval_set) + (None,))[:4]
        ey = np.asarray(ey, dtype=np.float32)
        ewt = np.ones(len(ey), np.float32) if ew is None else np.asarray(ew, dtype=np.float32)
        epred = np.asarray(eval_pred, dtype=np.float32).copy()
        eg0 = W.residuals(epred, ey, "eval label")
        ewt = W.check_weights(ewt, "eval weight")
        ehq = W.hess_fixed(ewt)
        eS0, eW = W.weighted_sum(eg0, ehq)
        eval_sums = [eS0]
    else:
        assert patience == 0
        eval_sums, eW, epred = None, None, None
    S0, Wsum = W.weighted_sum(g0, hq)
    train_sums = [S0]
    trees, preds, epreds, bags, feats = [], [pred.copy()], [epred.copy() if epred is not None else None], [], []
    run, best = rounds, 0
    for r in range(rounds):
        g = W.residuals(pred, y)                        # every row, in or out of the bag
        q = W.grad_fixed(g, wt)
        in_bag = bag(seed, tree0 + r, n, subsample)
        kept = features(seed, tree0 + r, num_feature, colsample_bytree)
        qb, hb = np.where(in_bag, q, 0).astype(np.int64), np.where(in_bag, hq, 0).astype(np.uint64)
        if int(hb.astype(object).sum()) == 0:
            raise ValueError("bag: the bag of round %d holds no weight" % (r + 1))
        t, pos = W.grow_tree(bins, qb, hb, emptied_cuts(cuts, num_feature, kept), max_depth, eta, lam, gamma, min_child_weight)
        # the node's value is the cut of the ORIGINAL list: the emptied one keeps the kept features' values in order
        pred = pred + t["value"][pos]
        assert pred.dtype == np.float32
        trees.append(t)
        bags.append(in_bag)
        feats.append(kept)
        preds.append(pred.copy())
        train_sums.append(W.weighted_sum(W.residuals(pred, y), hq)[0])
        if eval_set is not None:
            epred = epred + E.walk(t, ex, emissing)
            assert epred.dtype == np.float32
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
            "bags": bags, "features": feats}
