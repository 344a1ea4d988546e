"""Shared by the tests of boosting with a held-out set: a restatement of OHXBoosterBoostTreesEval in numpy and Python
integers, written from the text of include/ohxgb.h alone.  Nothing here calls the code under test.

The trees and the training margins after every round are grow_support.boost's; the held-out rows walk every restated
tree by their float values (x < value goes left, NaN or `missing` or a column the matrix lacks takes the default); the
sums are Python ints; the stop rule is a plain loop; the RMSE is math.sqrt(float(S) * 2.0**-48 / n) - float() of a Python
int rounds to nearest even."""
import math

import numpy as np

from tests import grow_support as G
from tests import refit_support as R


def walk(tree, x, missing):
    """The leaf value of every row of x (float32 [n][ncol]) in a restated tree."""
    x = np.asarray(x, dtype=np.float32)
    n, ncol = x.shape
    pos = np.zeros(n, dtype=np.int64)
    left, right = tree["left"].astype(np.int64), tree["right"].astype(np.int64)
    while True:
        inner = left[pos] >= 0
        if not inner.any():
            break
        rows = np.flatnonzero(inner)
        p = pos[rows]
        f = tree["feature"][p].astype(np.int64)
        have = f < ncol
        v = np.where(have, x[rows, np.where(have, f, 0)], np.float32(np.nan)).astype(np.float32)
        miss = np.isnan(v)
        if not np.isnan(missing):
            miss |= v == np.float32(missing)
        with np.errstate(invalid="ignore"):
            go_left = np.where(miss, tree["default_left"][p] != 0, v < tree["value"][p])
        pos[rows] = np.where(go_left, left[p], right[p])
    return tree["value"][pos].astype(np.float32)


def sum_squares(pred, y, what="label"):
    """S = sum q^2 as a Python int; raises ValueError where the call is refused for a residual out of range."""
    pred, y = np.asarray(pred, dtype=np.float32), np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        g = pred - y
    assert g.dtype == np.float32
    if not (np.all(np.isfinite(g)) and np.all(np.abs(g) < R.MAX_ABS_GRAD)):
        raise ValueError(f"{what}: a residual is not finite or reaches 256")
    scaled = g * R.SCALE
    assert scaled.dtype == np.float32
    return sum(int(q) * int(q) for q in np.rint(scaled).astype(np.int64))


def rmse(S, n):
    return math.sqrt(float(S) * 2.0 ** -48 / n)


def stop_rule(S, rounds, patience):
    """S: the held-out sums after 0 .. rounds trees (a callable t -> int, so that later rounds need not exist).
    -> (rounds_run, best)."""
    best = 0
    for t in range(1, rounds + 1):
        if S(t) < S(best):
            best = t
        if patience >= 1 and t - best >= patience:
            return t, best
    return rounds, best


def boost_eval(pred, x, missing, y, cuts, num_feature, eval_set=None, eval_pred=None, rounds=1, patience=0, **kw):
    """pred / eval_pred: the float32 margins of the forest so far over the training and the held-out rows;
    eval_set = (rows, missing, labels) or None.  -> dict: trees (the kept ones), all_trees, train_rmse, eval_rmse (lists of
    float, entries 0 .. rounds_run; eval_rmse None without a held-out set), train_sums, eval_sums (Python ints),
    rounds_run, best_round, nodes_added, pred and eval_pred after the kept trees."""
    out = G.boost(pred, x, missing, y, cuts, num_feature, rounds=rounds, **kw)
    preds = [np.asarray(pred, dtype=np.float32)] + out["preds"]
    if eval_set is not None:
        ex, emissing, ey = eval_set
        epreds = [np.asarray(eval_pred, dtype=np.float32).copy()]
        for t in out["trees"]:
            nxt = epreds[-1] + walk(t, ex, emissing)
            assert nxt.dtype == np.float32
            epreds.append(nxt)
        cache = {}

        def S(t):
            if t not in cache:
                cache[t] = sum_squares(epreds[t], ey, "eval label")
            return cache[t]
        run, best = stop_rule(S, rounds, patience)
        eval_sums = [S(t) for t in range(run + 1)]
    else:
        assert patience == 0
        run, best, eval_sums, epreds = rounds, rounds, None, None
    train_sums = [sum_squares(preds[t], y) for t in range(run + 1)]
    keep = best if (patience >= 1) else rounds
    trees = out["trees"][:keep]
    return {"trees": trees, "all_trees": out["trees"], "train_sums": train_sums, "eval_sums": eval_sums,
            "train_rmse": [rmse(s, len(preds[0])) for s in train_sums],
            "eval_rmse": [rmse(s, len(epreds[0])) for s in eval_sums] if eval_sums is not None else None,
            "rounds_run": run, "best_round": best, "nodes_added": sum(len(t["left"]) for t in trees),
            "pred": preds[keep], "eval_pred": epreds[keep] if epreds is not None else None}
