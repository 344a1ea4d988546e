"""Shared by the tests of trees deeper than eight levels (OHXBoosterBoostTreesDeep).  The restatement of the call is
grow_weighted_support.boost_weighted, which loops over the levels with no cap: the header says the Deep call is the
Weighted call word for word with max_depth up to 18.  What is added here are the common inputs of the cases and a view
of a restated tree level by level.  Nothing here calls the code under test."""
import functools

import numpy as np

from tests import grow_support as G
from tests import grow_weighted_support as W

MAX_DEPTH = 18
BASE = 0.5          # the margin of grow_support.empty_model: the model of every case has no tree


def boost_deep(pred, x, missing, y, w, cuts, num_feature, **kw):
    """grow_weighted_support.boost_weighted, max_depth in 1..18."""
    assert 1 <= kw.get("max_depth", 6) <= MAX_DEPTH
    return W.boost_weighted(pred, x, missing, y, w, cuts, num_feature, **kw)


def inputs(n, seed, nfeat=3, bins=255, missing=float("nan")):
    """-> (x float32 [n][nfeat] standard normal with 5 % missing, y = sin(3 x0) + 0.3 noise as float32, the quantile cuts
    of x by grow_support.quantile_cuts).  A missing x0 counts as 0 in the label."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, nfeat)).astype(np.float32)
    x0 = x[:, 0].copy()
    x[rng.random((n, nfeat)) < 0.05] = missing
    y = (np.sin(3.0 * x0) + 0.3 * rng.standard_normal(n)).astype(np.float32)
    return x, y, G.quantile_cuts(x, missing, bins)


def levels(t):
    """A restated tree level by level -> a list of (open nodes, splits): the nodes of level d, and how many of them
    split.  Node ids of a level are contiguous and ascend (allocation order), which is asserted."""
    out, level = [], [0]
    while level:
        assert level == list(range(level[0], level[0] + len(level))), "a level's ids are contiguous and ascending"
        split = [n for n in level if t["left"][n] >= 0]
        out.append((len(level), len(split)))
        level = [c for n in split for c in (int(t["left"][n]), int(t["right"][n]))]
    return out


def depth_of(t):
    """The deepest level that holds a node."""
    return len(levels(t)) - 1


@functools.lru_cache(maxsize=None)
def restated(n, seed, max_depth, bins, lam, mcw, rounds=1, nfeat=3, weighted=False, held_out=0, patience=0):
    """One restated case on the common inputs, shared by the tests that need it (the result is not to be changed).
    weighted: weights drawn from {0, 0.5, .., 2}; held_out: that many held-out rows from seed + 1 with the same cuts.
    -> (x, y, w, cuts, ev or None, the dict of boost_weighted)."""
    x, y, cuts = inputs(n, seed, nfeat, bins)
    rng = np.random.default_rng(seed + 7)
    w = rng.choice(np.arange(0.0, 2.5, 0.5).astype(np.float32), n) if weighted else None
    ev = None
    if held_out:
        ex, ey, _ = inputs(held_out, seed + 1, nfeat, bins)
        ew = rng.choice(np.arange(0.0, 2.5, 0.5).astype(np.float32), held_out) if weighted else None
        ev = (ex, float("nan"), ey, ew)
    want = boost_deep(np.full(n, BASE, np.float32), x, float("nan"), y, w, cuts, nfeat, eval_set=ev,
                      eval_pred=np.full(held_out, BASE, np.float32) if held_out else None, rounds=rounds, patience=patience,
                      max_depth=max_depth, eta=0.5, lam=lam, gamma=0.0, min_child_weight=mcw)
    return x, y, w, cuts, ev, want


def leaf_ids(t, x, missing=float("nan")):
    """The node every row of x ends on in the restated tree t, by the float walk of the header (x < value goes left, a
    missing value goes where default_left says; a column x lacks is missing) -> int32 [nrow]."""
    x = np.asarray(x, dtype=np.float32)
    n, ncol = x.shape
    pos = np.zeros(n, dtype=np.int64)
    for _ in range(MAX_DEPTH + 1):
        inner = t["left"][pos] >= 0
        if not inner.any():
            break
        f = t["feature"][pos].astype(np.int64)
        v = np.where(f < ncol, x[np.arange(n), np.minimum(f, ncol - 1)], np.float32("nan"))
        miss = np.isnan(v) if np.isnan(missing) else (np.isnan(v) | (v == np.float32(missing)))
        go_left = np.where(miss, t["default_left"][pos] != 0, v < t["value"][pos])
        pos = np.where(inner, np.where(go_left, t["left"][pos], t["right"][pos]), pos)
    assert np.all(t["left"][pos] < 0)
    return pos.astype(np.int32)
