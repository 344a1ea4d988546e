"""Shared by the tests of "ohx_interaction_constraints": a restatement in numpy and Python sets of the parameter's grammar,
of the sets P and A of a node and of a boost call that grows its trees under them, written from the text of
include/ohxgb.h alone, and an auditor of saved trees.  Nothing here calls the code under test.

A tree is grown by the level loop of grow_weighted_support.grow_tree and grow_mono_support.tree_grower, every node with
the features on its path (P) and those it may split on (A): a node's candidates are those of the other restatements'
best_split with the cut counts of the features outside A set to 0, so the candidates, their order, the ties, the gain form,
min_child_weight and the node numbering are theirs by construction.  A boost call is grow_reg_support.boost itself, run over
a copy of that module's globals in which `tree_grower` is this one (the module is not touched): the pairs, the bag, the
lists, the metrics and the stop rule are the regularised call's.  With inactive constraints it is grow_mono_support.boost
unchanged."""
import functools
import json
import re
import types

import numpy as np

from tests import grow_mono_support as M
from tests import grow_objective_support as O
from tests import grow_reg_support as RG
from tests import grow_support as G
from tests import grow_weighted_support as W

F32 = np.float32
INF = M.INF
BASE = O.BASE
NFEAT = 6
MAX_GROUPS, MAX_FEATURES = 64, 128
TWO_GROUPS = ((0, 1, 2), (3, 4, 5))
OVERLAP = ((0, 1), (1, 2, 3))              # features 4 and 5 are in no group
SINGLETONS = tuple((f,) for f in range(NFEAT))


# ---- the parameter ----

BLANK = r"[ \t]*"
ID = r"[0-9]+"
GROUP = r"\[" + BLANK + ID + "(?:" + BLANK + "," + BLANK + ID + ")*" + BLANK + r"\]"
GRAMMAR = re.compile(BLANK + r"\[" + BLANK + "(?:" + GROUP + "(?:" + BLANK + "," + BLANK + GROUP + ")*)?" + BLANK + r"\]" + BLANK)


def parse(value):
    """The header's grammar -> the groups as sorted lists of ids; ValueError for anything else."""
    if GRAMMAR.fullmatch(value) is None:
        raise ValueError("ohx_interaction_constraints: not a list of groups of ids in brackets")
    groups = [[int(i) for i in re.findall(ID, g)] for g in re.findall(GROUP, value)]
    if len(groups) > MAX_GROUPS:
        raise ValueError("ohx_interaction_constraints: more than 64 groups")
    for g in groups:
        if len(set(g)) != len(g) or max(g) >= MAX_FEATURES:
            raise ValueError("ohx_interaction_constraints: an id twice in a group, or an id of 128 or more")
    return [sorted(g) for g in groups]


def text(groups):
    return "[" + ",".join("[" + ",".join(str(int(f)) for f in g) + "]" for g in groups) + "]"


def active(groups, num_feature):
    """Constraints are inactive when the list is empty or when some group holds every feature."""
    every = set(range(num_feature))
    return len(groups) > 0 and not any(every <= set(g) for g in groups)


# ---- the sets ----

def allowed(path, groups, num_feature):
    """A of a node whose path has split on the features `path`: every feature at the root, else the path's own features and
    every group that holds them all."""
    path = set(path)
    if not path:
        return set(range(num_feature))
    out = set(path)
    for g in groups:
        if path <= set(g):
            out |= set(g)
    return out


# ---- a tree ----

def _reg_best_split(alpha, m):
    g = dict(W.__dict__)
    g["gain"] = lambda Gs, H, lam: RG.gain(Gs, H, lam, alpha, m)
    return types.FunctionType(W.best_split.__code__, g, "best_split")


def tree_grower(groups, alpha, m, constraints=None, seen=None):
    """-> grow_tree(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight) -> (tree, pos).  constraints: None (the
    regularised policy, which at alpha == 0 and m == 0 is the fixed-point one bit for bit) or an entry a feature (the
    monotone policy).  seen: a list that receives (G, H, base_weight) of every node, in node order.  The tree carries "path"
    and "allowed", a set a node."""
    reg_split = _reg_best_split(alpha, m)

    def grow_tree(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight):
        cut_ptr, cut_values = cuts
        F, n = bins.shape
        ncuts = [int(cut_ptr[f + 1]) - int(cut_ptr[f]) for f in range(F)]
        pos = np.zeros(n, dtype=np.int64)
        nodes = [dict(G=int(q.sum()), H=int(hq.astype(object).sum()), parent=-1, lo=-INF, hi=INF, P=frozenset(), A=frozenset(range(F)))]
        level = [0]
        for _ in range(max_depth):
            nxt = []
            for p in level:
                nd = nodes[p]
                rows = np.flatnonzero(pos == p)
                Gh = np.zeros((F, 256), dtype=np.int64)
                Hh = np.zeros((F, 256), dtype=np.uint64)
                mine = [ncuts[f] if f in nd["A"] else 0 for f in range(F)]      # the candidates: f additionally in A(p)
                for f in range(F):
                    if mine[f]:
                        np.add.at(Gh[f], bins[f, rows], q[rows])
                        np.add.at(Hh[f], bins[f, rows], hq[rows])
                if constraints is None:
                    best = reg_split(Gh, Hh, mine, nd["G"], nd["H"], lam, min_child_weight)
                else:
                    best = M.best_split(Gh, Hh, mine, nd["G"], nd["H"], lam, min_child_weight, alpha, m, nd["lo"], nd["hi"], constraints)
                if best is None or not best[0] > float(F32(gamma)):
                    continue
                loss, f, j, dl, GL, HL = best[:6]
                assert f in nd["A"]
                left = len(nodes)
                ivL = ivR = (nd["lo"], nd["hi"])
                if constraints is not None:
                    ivL, ivR = M.children(constraints[f], best[6], best[7], nd["lo"], nd["hi"])
                path = nd["P"] | {f}
                may = frozenset(allowed(path, groups, F))
                nd.update(left=left, right=left + 1, feature=f, j=j, dl=dl, loss=loss)
                nodes.append(dict(G=GL, H=HL, parent=p + G.LEFT_BIT, lo=ivL[0], hi=ivL[1], P=path, A=may))
                nodes.append(dict(G=nd["G"] - GL, H=nd["H"] - HL, parent=p, lo=ivR[0], hi=ivR[1], P=path, A=may))
                b = bins[f, rows]
                go_left = np.where(b == W.MISSING_BIN, bool(dl), b <= j)
                pos[rows] = np.where(go_left, left, left + 1)
                nxt += [left, left + 1]
            level = nxt
        k = len(nodes)
        t = {"left": np.full(k, -1, np.int32), "right": np.full(k, -1, np.int32), "parent": np.zeros(k, np.int32),
             "feature": np.zeros(k, np.uint32), "default_left": np.zeros(k, np.uint32), "value": np.zeros(k, F32),
             "loss_chg": np.zeros(k, F32), "sum_hess": np.zeros(k, F32), "base_weight": np.zeros(k, F32)}
        for i, nd in enumerate(nodes):
            if constraints is None:
                leaf, w, sh = RG.solve(nd["G"], nd["H"], eta, lam, alpha, m)
            else:
                leaf, w, sh = M.solve(nd["G"], nd["H"], eta, lam, alpha, m, nd["lo"], nd["hi"])
            if seen is not None:
                seen.append((nd["G"], nd["H"], w))
            t["parent"][i] = nd["parent"]
            t["sum_hess"][i] = sh
            t["base_weight"][i] = w
            if "left" in nd:
                t["left"][i], t["right"][i] = nd["left"], nd["right"]
                t["feature"][i], t["default_left"][i] = nd["feature"], nd["dl"]
                t["value"][i] = cut_values[int(cut_ptr[nd["feature"]]) + nd["j"]]
                t["loss_chg"][i] = F32(nd["loss"])
            else:
                t["value"][i] = leaf
        t["path"] = [nd["P"] for nd in nodes]
        t["allowed"] = [nd["A"] for nd in nodes]
        return t, pos

    return grow_tree


# ---- a boost call ----

def boost(groups, constraints, objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw):
    """grow_reg_support.boost under the groups, and under the monotone constraints where one is not 0.  -> its dict."""
    if any(f >= num_feature for g in groups for f in g):
        raise ValueError("ohx_interaction_constraints: an id that is no feature of the booster")
    if not active(groups, num_feature):
        return M.boost(constraints, objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw)
    cons = M.padded(constraints, num_feature)
    cons = cons if M.active(cons) else None
    g = dict(RG.__dict__)
    g["tree_grower"] = lambda a, mm, seen=None: tree_grower(groups, a, mm, cons, seen)
    constrained = types.FunctionType(RG.boost.__code__, g, "boost", RG.boost.__defaults__)
    return constrained(objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw)


def inputs(n, seed, bins=64, held_out=0):
    """grow_objective_support.inputs with six features and 1.5 x0 x3 added to the labels (a missing value counts as 0): a
    product of a feature of TWO_GROUPS' first group with one of its second, so a free tree mixes the groups."""
    x, y, w, cuts, ev = O.inputs(n, seed, NFEAT, bins, held_out)

    def crossed(rows, labels):
        r = np.nan_to_num(rows, nan=0.0)
        out = labels + F32(1.5) * r[:, 0] * r[:, 3]
        assert out.dtype == F32
        return out

    if ev is not None:
        ev = (ev[0], ev[1], crossed(ev[0], ev[2]), ev[3])
    return x, crossed(x, y), w, cuts, ev


@functools.lru_cache(maxsize=None)
def restated(groups, n, seed, max_depth, constraints=(), objective="squarederror", slope=1.0, alpha=0.0, m=0.0, metric="rmse", bins=64,
             rounds=2, held_out=0, patience=0, subsample=1.0, colsample=1.0, draw_seed=0, lam=1.0, mcw=0.0, eta=0.125, gamma=0.0):
    """One restated case on `inputs`, computed once and shared (the result is not to be changed).  groups: a tuple of tuples.
    -> (x, y, w, cuts, ev, the dict of boost)."""
    x, y, w, cuts, ev = inputs(n, seed, bins, held_out)
    want = boost(groups, constraints, objective, slope, alpha, m, metric, np.full(n, BASE, F32), x, float("nan"), y, w, cuts, NFEAT,
                 eval_set=ev, eval_pred=np.full(held_out, BASE, F32) if held_out else None, rounds=rounds, patience=patience,
                 max_depth=max_depth, eta=eta, lam=lam, gamma=gamma, min_child_weight=mcw, subsample=subsample,
                 colsample_bytree=colsample, seed=draw_seed)
    return x, y, w, cuts, ev, want


# ---- the auditor ----

def _trees_of_any(image):
    """(left, right, feature) arrays of every tree of a saved model in any of the three formats, by the library's own
    conversion to JSON where the image is not JSON."""
    from quickchem_amd import synth
    data = bytes(image)
    try:
        json.loads(data.decode())
    except (UnicodeDecodeError, ValueError):
        data = bytes(synth.convert_model(data, "json"))
    return [(t["left"], t["right"], t["feature"]) for t in G.trees_of(data)]


def tree_violations(left, right, feature, groups, num_feature):
    """The split nodes of one tree whose feature is not in the A derived from the features of their ancestors -> a list of
    (node, feature, sorted A)."""
    bad = []
    stack = [(0, frozenset())]
    while stack:
        p, path = stack.pop()
        if int(left[p]) < 0:
            continue
        f = int(feature[p])
        may = allowed(path, groups, num_feature)
        if f not in may:
            bad.append((p, f, sorted(may)))
        below = path | {f}
        stack += [(int(left[p]), below), (int(right[p]), below)]
    return sorted(bad)


def violations(image_or_trees, groups, num_feature, first=0):
    """C2 over the trees from `first` on of a saved model (bytes in any format) or of a list of restated trees
    -> a list of (tree, node, feature, sorted A)."""
    if isinstance(image_or_trees, (bytes, bytearray, memoryview)):
        trees = _trees_of_any(image_or_trees)
    else:
        trees = [(t["left"], t["right"], t["feature"]) for t in image_or_trees]
    return [(i,) + v for i, (le, ri, fe) in enumerate(trees) if i >= first for v in tree_violations(le, ri, fe, groups, num_feature)]


def path_features(left, right, feature):
    """The set of features on every root-to-leaf path of one tree."""
    out = []
    stack = [(0, frozenset())]
    while stack:
        p, path = stack.pop()
        if int(left[p]) < 0:
            out.append(path)
            continue
        below = path | {int(feature[p])}
        stack += [(int(left[p]), below), (int(right[p]), below)]
    return out
