"""Shared by the tests of row and column subsampling for trees deeper than eight levels
(OHXBoosterBoostTreesDeepSampled).  The restatement of the call is grow_sampled_support.boost_sampled, whose level loop
has no cap: the header says the call is the Sampled call word for word with max_depth up to 18.  What is added here are
the common inputs of the cases (grow_deep_support.inputs) and a cached case.  Nothing here calls the code under test."""
import functools

import numpy as np

from tests import grow_deep_support as D
from tests import grow_sampled_support as P

MAX_DEPTH = D.MAX_DEPTH
BASE = D.BASE       # the margin of grow_support.empty_model: the model of every case has no tree


def boost_deep_sampled(pred, x, missing, y, w, cuts, num_feature, **kw):
    """grow_sampled_support.boost_sampled, max_depth in 1..18."""
    assert 1 <= kw.get("max_depth", 6) <= MAX_DEPTH
    return P.boost_sampled(pred, x, missing, y, w, cuts, num_feature, **kw)


@functools.lru_cache(maxsize=None)
def restated(n, seed, max_depth, bins, lam, mcw, subsample, colsample, draw_seed, rounds=1, nfeat=3, weighted=False,
             held_out=0, patience=0, tree0=0):
    """One restated case on the common inputs, shared by the tests that need it (the result is not to be changed).
    weighted: weights drawn from {0, 0.5, .., 2}; held_out: that many held-out rows from seed + 1 with the same cuts.
    -> (x, y, w, cuts, ev or None, the dict of boost_sampled)."""
    x, y, cuts = D.inputs(n, seed, nfeat, bins)
    rng = np.random.default_rng(seed + 7)
    w = rng.choice(np.arange(0.0, 2.5, 0.5).astype(np.float32), n) if weighted else None
    ev = None
    if held_out:
        ex, ey, _ = D.inputs(held_out, seed + 1, nfeat, bins)
        ew = rng.choice(np.arange(0.0, 2.5, 0.5).astype(np.float32), held_out) if weighted else None
        ev = (ex, float("nan"), ey, ew)
    want = boost_deep_sampled(np.full(n, BASE, np.float32), x, float("nan"), y, w, cuts, nfeat, eval_set=ev,
                              eval_pred=np.full(held_out, BASE, np.float32) if held_out else None, rounds=rounds,
                              patience=patience, max_depth=max_depth, eta=0.5, lam=lam, gamma=0.0, min_child_weight=mcw,
                              subsample=subsample, colsample_bytree=colsample, seed=draw_seed, tree0=tree0)
    return x, y, w, cuts, ev, want
