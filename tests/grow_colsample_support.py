"""Shared by the tests of "ohx_colsample_bylevel" and "ohx_colsample_bynode": a restatement in numpy uint64 (which wraps)
and Python integers of the level and node keys, of n_lvl and n_node, of S_lvl(d) and S_node(p), written from the text of
include/ohxgb.h alone, and of a boost call that grows its trees over them.  Nothing here calls the code under test.

A tree is grown by the existing growers themselves - grow_weighted_support.grow_tree under grow_reg_support's policy, or
grow_mono_support's under an active constraint - run over a copy of their globals in which `best_split` is the grower's
own, asked with the cut counts of every feature outside S_node(p) set to 0: such a feature has no candidate, and the
candidates of the others, their order, the ties and the node numbering are the growers' by construction.  The modules are
not touched.  The node at hand is followed from outside: the growers ask for the nodes of a level in ascending id, once
each, and a node that splits takes the next two ids.  A boost call is grow_reg_support.boost run over a copy of that
module's globals that hands over this grower and notes the tree's index and list; the pairs, the bag, the tree's list,
the metrics and the stop rule are therefore the regularised call's."""
import functools
import math
import types

import numpy as np

from tests import grow_mono_support as M
from tests import grow_objective_support as O
from tests import grow_reg_support as RG
from tests import grow_sampled_support as P

F32 = np.float32
BASE = O.BASE
NODE_KEY_BASE = 32


# ---- the draws ----

def _u64(v):
    return np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


def level_key(seed, i, d):
    """K_lvl(i, d) = mix(K_col(i) + gamma64 * (d + 1))."""
    with np.errstate(over="ignore"):
        return P.mix(P.col_key(seed, i) + P.GAMMA64 * _u64(d + 1))


def node_key(seed, i, p):
    """K_node(i, p) = mix(K_col(i) + gamma64 * (32 + p))."""
    with np.errstate(over="ignore"):
        return P.mix(P.col_key(seed, i) + P.GAMMA64 * _u64(NODE_KEY_BASE + p))


def fraction(v, name):
    """The parameter as the handle keeps it: a float32, finite, 0 < v <= 1."""
    v = F32(v)
    if not (np.isfinite(v) and v > 0 and v <= 1):
        raise ValueError(f"{name}: not finite, <= 0 or > 1")
    return v


def count(frac, n, name="fraction"):
    """max(1, (int) floor((double)frac * n))."""
    return max(1, int(math.floor(float(np.float64(fraction(frac, name))) * n)))


def feature_keys(key, features):
    """mix(key + f) of every f, as Python ints."""
    with np.errstate(over="ignore"):
        return [int(k) for k in P.mix(key + np.asarray(list(features), dtype=np.uint64))]


def smallest(keys, features, take):
    """The `take` features smallest by (key, f), ascending in f."""
    order = sorted((int(k), int(f)) for k, f in zip(keys, features))
    return sorted(f for _, f in order[:take])


def level_features(seed, i, d, tree_list, bylevel):
    """S_lvl(d) of tree i, ascending."""
    tree_list = [int(f) for f in tree_list]
    n_lvl = count(bylevel, len(tree_list), "ohx_colsample_bylevel")
    if n_lvl == len(tree_list):
        return tree_list
    return smallest(feature_keys(level_key(seed, i, d), tree_list), tree_list, n_lvl)


def node_features(seed, i, p, level_list, bynode):
    """S_node(p) of tree i over its level's list, ascending."""
    level_list = [int(f) for f in level_list]
    n_node = count(bynode, len(level_list), "ohx_colsample_bynode")
    if n_node == len(level_list):
        return level_list
    return smallest(feature_keys(node_key(seed, i, p), level_list), level_list, n_node)


def draws_nothing(n_sel, bylevel, bynode):
    n_lvl = count(bylevel, n_sel)
    return n_lvl == n_sel and count(bynode, n_lvl) == n_lvl


# ---- a tree ----

class Follower:
    """Which node the grower asks about: the nodes of a level in ascending id, once each; one that splits takes the next
    two ids.  at() -> (p, d); step(split) moves on."""

    def __init__(self):
        self.level, self.nxt, self.k, self.d, self.nodes = [0], [], 0, 0, 1

    def at(self):
        return self.level[self.k], self.d

    def step(self, split):
        if split:
            self.nxt += [self.nodes, self.nodes + 1]
            self.nodes += 2
        self.k += 1
        if self.k == len(self.level):
            self.level, self.nxt, self.k, self.d = self.nxt, [], 0, self.d + 1


def tree_grower(alpha, m, constraints, seen, seed, i, tree_list, bylevel, bynode, log):
    """-> grow_tree(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight) -> (tree, pos): the regularised grower,
    or the constrained one where `constraints` (an entry a feature) is active, with the candidates of node p filtered to
    S_node(p).  log receives a dict a node asked about: p, d, level (S_lvl), node (S_node), feature (the split's, or None),
    free (the feature of the best candidate over S_tree where that would split, else None)."""
    constrained = M.active(constraints)
    base = M.tree_grower(alpha, m, list(constraints), seen) if constrained else RG.tree_grower(alpha, m, seen)

    def grow_tree(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight):
        g = dict(base.__globals__)
        inner = g["best_split"]
        follow = Follower()
        levels = {}
        floor = float(F32(gamma))

        def best_split(Gh, Hh, ncuts, *rest):
            p, d = follow.at()
            if d not in levels:
                levels[d] = level_features(seed, i, d, tree_list, bylevel)
            mine = node_features(seed, i, p, levels[d], bynode)
            best = inner(Gh, Hh, [n if f in mine else 0 for f, n in enumerate(ncuts)], *rest)
            free = inner(Gh, Hh, ncuts, *rest)          # (the cuts are the tree's already: emptied outside S_tree)
            split = best is not None and best[0] > floor
            log.append(dict(p=p, d=d, level=levels[d], node=mine, feature=best[1] if split else None,
                            free=free[1] if free is not None and free[0] > floor else None))
            follow.step(split)
            return best

        g["best_split"] = best_split
        grower = types.FunctionType(base.__code__, g, "grow_tree", base.__defaults__, base.__closure__)
        t, pos = grower(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight)
        assert follow.nodes == len(t["left"]), "the follower numbered the nodes as the grower did"
        return t, pos

    return grow_tree


# ---- a boost call ----

def boost(bylevel, bynode, constraints, objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw):
    """grow_reg_support.boost (grow_mono_support.boost under active constraints) with both fractions.  -> its dict, with
    "draws": per tree grown the log of tree_grower.  Fractions that take no feature away give the other module's call."""
    fraction(bylevel, "ohx_colsample_bylevel")
    fraction(bynode, "ohx_colsample_bynode")
    cons = M.padded(constraints, num_feature)
    n_sel = P.num_selected(num_feature, kw.get("colsample_bytree", 1.0))
    if draws_nothing(n_sel, bylevel, bynode):
        out = M.boost(constraints, objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw)
        return dict(out, draws=None)
    at, draws = {}, []

    def features(seed, i, F, colsample):
        kept = P.features(seed, i, F, colsample)
        at.update(seed=seed, i=i, kept=kept)
        return kept

    def grower(a, mm, seen=None):
        draws.append([])
        return tree_grower(a, mm, cons, seen, at["seed"], at["i"], at["kept"], bylevel, bynode, draws[-1])

    g = dict(RG.__dict__)
    g["P"] = types.SimpleNamespace(**dict({k: v for k, v in vars(P).items() if not k.startswith("__")}, features=features))
    g["tree_grower"] = grower
    call = types.FunctionType(RG.boost.__code__, g, "boost", RG.boost.__defaults__)
    out = call(objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw)
    return dict(out, draws=draws)


def narrowed(draws):
    """How many nodes of the logs `draws` have their unrestricted winner outside S_node(p): without the filter such a node
    splits otherwise."""
    return sum(1 for log in draws for e in log if e["free"] is not None and e["free"] not in e["node"])


@functools.lru_cache(maxsize=None)
def restated(bylevel, bynode, constraints, objective, slope, alpha, m, metric, n, seed, max_depth, bins=64, nfeat=3, rounds=2,
             held_out=0, patience=0, subsample=1.0, colsample=1.0, draw_seed=0, lam=1.0, mcw=0.0, weighted=True, eta=0.125, gamma=0.0,
             tree0=0):
    """One restated case on grow_objective_support.inputs, computed once and shared (the result is not to be changed).
    constraints: a tuple.  -> (x, y, w, cuts, ev, the dict of boost)."""
    x, y, w, cuts, ev = O.inputs(n, seed, nfeat, bins, held_out)
    if not weighted:
        w = None
        ev = (ev[0], ev[1], ev[2], None) if ev is not None else None
    want = boost(bylevel, bynode, constraints, objective, slope, alpha, m, metric, np.full(n, BASE, F32), x, float("nan"), y, w, cuts,
                 nfeat, eval_set=ev, eval_pred=np.full(held_out, BASE, F32) if held_out else None, rounds=rounds, patience=patience,
                 max_depth=max_depth, eta=eta, lam=lam, gamma=gamma, min_child_weight=mcw, subsample=subsample,
                 colsample_bytree=colsample, seed=draw_seed, tree0=tree0)
    return x, y, w, cuts, ev, want
