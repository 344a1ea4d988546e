"""Shared by the tests of "ohx_monotone_constraints": a restatement in numpy and Python floats and integers of the weight
under an interval, of gain_w, of a constrained node's split and of the tree grown with them, written from the text of
include/ohxgb.h alone, and of a boost call that grows its trees so.  Nothing here calls the code under test.

The policy is Python floats (IEEE doubles) in the header's order, one rounding an operation.  A boost call is
grow_reg_support.boost itself, run over a copy of that module's globals in which `tree_grower` is the constrained one
(the module is not touched): the pairs, the bag, the lists, the metrics and the stop rule are therefore the regularised
call's by construction.  With no active constraint it is grow_reg_support.boost unchanged."""
import functools
import math
import re
import types

import numpy as np

from tests import grow_eval_support as E
from tests import grow_objective_support as O
from tests import grow_reg_support as RG
from tests import grow_support as G
from tests import grow_weighted_support as W

F32 = np.float32
INF = math.inf
BASE = O.BASE
MAX_ENTRIES = 128


# ---- the parameter ----

TOKEN = r"(?:-1|\+1|0|1)"
BLANK = r"[ \t]*"
GRAMMAR = re.compile(BLANK + r"\(" + BLANK + "(?:" + TOKEN + "(?:" + BLANK + "," + BLANK + TOKEN + ")*)?" + BLANK + r"\)" + BLANK)


def parse(value):
    """The header's grammar -> the list of entries; ValueError for anything else."""
    if GRAMMAR.fullmatch(value) is None:
        raise ValueError("ohx_monotone_constraints: not a list of -1, 0, 1 or +1 in parentheses")
    entries = [int(e) for e in re.findall(TOKEN, value)]
    if len(entries) > MAX_ENTRIES:
        raise ValueError("ohx_monotone_constraints: more than 128 entries")
    return entries


def padded(constraints, num_feature):
    c = [int(v) for v in constraints]
    if len(c) > num_feature:
        raise ValueError("ohx_monotone_constraints: more entries than features")
    assert all(v in (-1, 0, 1) for v in c)
    return c + [0] * (num_feature - len(c))


def active(constraints):
    return any(int(v) != 0 for v in constraints)


# ---- the policy ----

def sums(Gs, H, lam):
    """(Gd, D) of the header."""
    return float(int(Gs)) * 2.0 ** -24, W.hess(H) + float(F32(lam))


def weight(Gs, H, lam, alpha, m, lo, hi):
    """w(G, H; lo, hi): the regularised weight, then the clamp as the header writes it."""
    Gd, D = sums(Gs, H, lam)
    w = RG.weight(Gd, D, float(F32(alpha)), float(F32(m)))
    return lo if w < lo else (hi if w > hi else w)


def gain_w(Gs, H, lam, alpha, w):
    Gd, D = sums(Gs, H, lam)
    return -((2.0 * Gd) * w + (D * w) * w) - (2.0 * float(F32(alpha))) * abs(w)


def solve(Gs, H, eta, lam, alpha, m, lo, hi):
    """(leaf, base_weight, sum_hess) float32."""
    w = F32(weight(Gs, H, lam, alpha, m, lo, hi))
    leaf = w * F32(eta)
    assert leaf.dtype == F32
    return leaf, w, F32(W.hess(H))


def children(c, wL, wR, lo, hi):
    """((lo_L, hi_L), (lo_R, hi_R)) of a split on a feature with constraint c."""
    if c == 0:
        return (lo, hi), (lo, hi)
    mid = (wL + wR) * 0.5
    return ((lo, mid), (mid, hi)) if c > 0 else ((mid, hi), (lo, mid))


def best_split(Gh, Hh, ncuts, Gp, Hp, lam, min_child_weight, alpha, m, lo, hi, constraints):
    """Gh int64 / Hh uint64 [F][256] -> None or (loss_chg, f, j, dl, GL, HL, wL, wR).  The candidates, their order and the
    existing rule are grow_weighted_support.best_split's."""
    mcw = float(F32(min_child_weight))
    if W.hess(Hp) < 2.0 * mcw:
        return None
    best = None
    parent = None
    for f in range(Gh.shape[0]):
        c = constraints[f]
        GLb = HLb = 0
        Gm, Hm = int(Gh[f, W.MISSING_BIN]), int(Hh[f, W.MISSING_BIN])
        for j in range(int(ncuts[f])):
            GLb += int(Gh[f, j])
            HLb += int(Hh[f, j])
            for dl in (0, 1):
                GL = GLb + (Gm if dl else 0)
                HL = HLb + (Hm if dl else 0)
                GR, HR = Gp - GL, Hp - HL
                if HL <= 0 or HR <= 0:
                    continue
                if W.hess(HL) < mcw or W.hess(HR) < mcw:
                    continue
                wL, wR = weight(GL, HL, lam, alpha, m, lo, hi), weight(GR, HR, lam, alpha, m, lo, hi)
                if not (c == 0 or (c > 0 and wL <= wR) or (c < 0 and wL >= wR)):
                    continue
                if parent is None:
                    parent = gain_w(Gp, Hp, lam, alpha, weight(Gp, Hp, lam, alpha, m, lo, hi))
                loss = (gain_w(GL, HL, lam, alpha, wL) + gain_w(GR, HR, lam, alpha, wR)) - parent
                if best is None or loss > best[0]:
                    best = (loss, f, j, dl, GL, HL, wL, wR)
    return best


def tree_grower(alpha, m, constraints, seen=None):
    """-> grow_tree(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight) -> (tree, pos): the level loop, the node
    numbering and the record of grow_weighted_support.grow_tree, every node with its interval.  `constraints` holds an
    entry a feature.  seen: a list that receives (G, H, base_weight) of every node, in node order."""

    def grow_tree(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight):
        cut_ptr, cut_values = cuts
        F, n = bins.shape
        assert len(constraints) == F
        ncuts = [int(cut_ptr[f + 1]) - int(cut_ptr[f]) for f in range(F)]
        pos = np.zeros(n, dtype=np.int64)
        nodes = [dict(G=int(q.sum()), H=int(hq.astype(object).sum()), parent=-1, lo=-INF, hi=INF)]
        level = [0]
        for _ in range(max_depth):
            nxt = []
            for p in level:
                nd = nodes[p]
                rows = np.flatnonzero(pos == p)
                Gh = np.zeros((F, 256), dtype=np.int64)
                Hh = np.zeros((F, 256), dtype=np.uint64)
                for f in range(F):
                    if ncuts[f]:          # (a feature without cuts has no candidate)
                        np.add.at(Gh[f], bins[f, rows], q[rows])
                        np.add.at(Hh[f], bins[f, rows], hq[rows])
                best = best_split(Gh, Hh, ncuts, nd["G"], nd["H"], lam, min_child_weight, alpha, m, nd["lo"], nd["hi"], constraints)
                if best is None or not best[0] > float(F32(gamma)):
                    continue
                loss, f, j, dl, GL, HL, wL, wR = best
                left = len(nodes)
                (loL, hiL), (loR, hiR) = children(constraints[f], wL, wR, nd["lo"], nd["hi"])
                nd.update(left=left, right=left + 1, feature=f, j=j, dl=dl, loss=loss)
                nodes.append(dict(G=GL, H=HL, parent=p + G.LEFT_BIT, lo=loL, hi=hiL))
                nodes.append(dict(G=nd["G"] - GL, H=nd["H"] - HL, parent=p, lo=loR, hi=hiR))
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
            leaf, w, sh = solve(nd["G"], nd["H"], eta, lam, alpha, m, nd["lo"], nd["hi"])
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
        t["intervals"] = [(nd["lo"], nd["hi"]) for nd in nodes]
        return t, pos

    return grow_tree


# ---- a boost call ----

def boost(constraints, objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw):
    """grow_reg_support.boost under the constraints (fewer than num_feature entries: 0 for the rest).  -> its dict."""
    cons = padded(constraints, num_feature)
    if not active(cons):
        return RG.boost(objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw)
    g = dict(RG.__dict__)
    g["tree_grower"] = lambda a, mm, seen=None: tree_grower(a, mm, cons, seen)
    constrained = types.FunctionType(RG.boost.__code__, g, "boost", RG.boost.__defaults__)
    return constrained(objective, slope, alpha, m, metric, pred, x, missing, y, w, cuts, num_feature, **kw)


@functools.lru_cache(maxsize=None)
def restated(constraints, objective, slope, alpha, m, metric, n, seed, max_depth, bins=64, nfeat=3, rounds=2, held_out=0, patience=0,
             subsample=1.0, colsample=1.0, draw_seed=0, lam=1.0, mcw=0.0, weighted=True, eta=0.125, gamma=0.0):
    """One restated case on grow_objective_support.inputs, computed once and shared (the result is not to be changed).
    constraints: a tuple.  -> (x, y, w, cuts, ev, the dict of boost)."""
    x, y, w, cuts, ev = O.inputs(n, seed, nfeat, bins, held_out)
    if not weighted:
        w = None
        ev = (ev[0], ev[1], ev[2], None) if ev is not None else None
    want = boost(constraints, objective, slope, alpha, m, metric, np.full(n, BASE, F32), x, float("nan"), y, w, cuts, nfeat,
                 eval_set=ev, eval_pred=np.full(held_out, BASE, F32) if held_out else None, rounds=rounds, patience=patience,
                 max_depth=max_depth, eta=eta, lam=lam, gamma=gamma, min_child_weight=mcw, subsample=subsample,
                 colsample_bytree=colsample, seed=draw_seed)
    return x, y, w, cuts, ev, want


def same_trees(a, b):
    """Two lists of restated trees hold the same arrays, bit for bit."""
    return len(a) == len(b) and all(np.asarray(s[k]).tobytes() == np.asarray(t[k]).tobytes() for s, t in zip(a, b) for k in G.ARRAYS)


# ---- the property ----

def sweep_values(cuts, f):
    """Every cut value of feature f and the midpoints between neighbouring cuts, ascending, float32."""
    cut_ptr, cut_values = cuts
    c = np.asarray(cut_values[int(cut_ptr[f]):int(cut_ptr[f + 1])], dtype=F32)
    mids = ((c[:-1].astype(np.float64) + c[1:].astype(np.float64)) * 0.5).astype(F32)
    return np.unique(np.concatenate([c, mids]))


def sweep_rows(base_rows, f, values):
    """[len(base_rows)][len(values)][ncol]: every base row with x_f swept over `values`."""
    rows = np.repeat(np.asarray(base_rows, dtype=F32)[:, None, :], len(values), axis=1)
    rows[:, :, f] = values[None, :]
    return rows


def tree_values(t, rows):
    """[rows][sweep] leaf values of the tree arrays `t` over sweep_rows' output, walked as xgboost walks (x < value goes
    left, a missing x follows default_left)."""
    r, k, ncol = rows.shape
    return E.walk(t, rows.reshape(r * k, ncol), float("nan")).reshape(r, k)


def violations(values, c):
    """How many neighbouring pairs of `values` [rows][sweep] stand against the direction c, compared exactly."""
    a, b = np.asarray(values)[:, :-1], np.asarray(values)[:, 1:]
    return int(np.count_nonzero(a > b if c > 0 else a < b))


# the inputs of the property test: y = sin(3 x0) + noise bends both ways in x0, so a free tree does too
PROPERTY = dict(n=1300, seed=281, nfeat=3, max_depth=6, rounds=2, constraints=(1, 0, -1), base_rows=32)


@functools.lru_cache(maxsize=None)
def property_case(constrained=True):
    """-> (x, y, w, cuts, the dict of boost) on the inputs of the property test, under PROPERTY's constraints or free."""
    p = PROPERTY
    x, y, w, cuts, _, want = restated(p["constraints"] if constrained else (), "squarederror", 1.0, 0.0, 0.0, "rmse", p["n"], p["seed"],
                                      p["max_depth"], nfeat=p["nfeat"], rounds=p["rounds"])
    return x, y, w, cuts, want


def property_sweeps(x, cuts):
    """{f: rows [base_rows][sweep][ncol]} for every constrained feature of PROPERTY."""
    return {f: sweep_rows(x[:PROPERTY["base_rows"]], f, sweep_values(cuts, f)) for f, c in enumerate(PROPERTY["constraints"]) if c}
