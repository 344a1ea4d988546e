"""Shared by the tests of boosting with row weights: a restatement of OHXBoosterBoostTreesWeighted in numpy and Python
integers and floats, written from the text of include/ohxgb.h alone.  Nothing here calls the code under test.

hq and q are made with np.float32 products and np.rint; the histograms are np.add.at on int64 / uint64; the hessian
sum becomes a double by float() of a Python int (round to nearest even) times 2.0**-24; the gains are Python floats
(IEEE double) in the stated order; the tie rule is a plain ascending loop over (f, j, dl) with a strict >; S and W are
Python ints; the RMSE is math.sqrt((float(S) * 2.0**-72) / (float(W) * 2.0**-24)).  Binning, the float walk of the
held-out rows and the stop rule are those of grow_support and grow_eval_support: the header refers to the same steps."""
import math

import numpy as np

from tests import grow_eval_support as E
from tests import grow_support as G
from tests import refit_support as R

MISSING_BIN = G.MISSING_BIN
MAX_WEIGHT = 256.0


def check_weights(w, what="weight"):
    w = np.asarray(w, dtype=np.float32)
    if not (np.all(np.isfinite(w)) and np.all(w >= 0) and np.all(w < np.float32(MAX_WEIGHT))):
        raise ValueError(f"{what}: not finite, negative or >= 256")
    return w


def hess_fixed(w):
    """hq = (uint64) rint(w * 2^24), the product in float32 (exact: a power of two)."""
    scaled = np.asarray(w, dtype=np.float32) * R.SCALE
    assert scaled.dtype == np.float32
    return np.rint(scaled).astype(np.uint64)


def residuals(pred, y, what="label"):
    """g = pred - y in float32; raises where it is not finite or reaches 256."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.asarray(pred, dtype=np.float32) - np.asarray(y, dtype=np.float32)
    assert g.dtype == np.float32
    if not (np.all(np.isfinite(g)) and np.all(np.abs(g) < R.MAX_ABS_GRAD)):
        raise ValueError(f"{what}: a residual is not finite or reaches 256")
    return g


def grad_fixed(g, w):
    """q = (int64) rint((g * w) * 2^24): one float32 multiply, then the exact scaling; raises "label" at |gw| >= 256."""
    gw = np.asarray(g, dtype=np.float32) * np.asarray(w, dtype=np.float32)
    assert gw.dtype == np.float32
    if not np.all(np.abs(gw) < R.MAX_ABS_GRAD):
        raise ValueError("label: a weighted gradient reaches 256")
    scaled = gw * R.SCALE
    assert scaled.dtype == np.float32
    return np.rint(scaled).astype(np.int64)


def hess(H):
    """Hd = (double)H * 2^-24."""
    return float(int(H)) * 2.0 ** -24


def gain(Gs, H, lam):
    Gd = float(int(Gs)) * 2.0 ** -24
    return (Gd * Gd) / (hess(H) + float(np.float32(lam)))


def solve(Gs, H, eta, lam):
    """(leaf, base_weight, sum_hess) float32."""
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.float32(np.float64(-(float(int(Gs)) * 2.0 ** -24)) / np.float64(hess(H) + float(np.float32(lam))))
    leaf = w * np.float32(eta)
    assert leaf.dtype == np.float32
    return leaf, w, np.float32(hess(H))


def best_split(Gh, Hh, ncuts, Gp, Hp, lam, min_child_weight):
    """Gh int64 / Hh uint64 [F][256] -> None or (loss_chg, f, j, dl, GL, HL); a node with Hd < 2 * min_child_weight has no
    candidate."""
    mcw = float(np.float32(min_child_weight))
    if hess(Hp) < 2.0 * mcw:
        return None
    best = None
    parent = None
    for f in range(Gh.shape[0]):
        nc = int(ncuts[f])
        GLb = HLb = 0
        for j in range(nc):
            GLb += int(Gh[f, j])
            HLb += int(Hh[f, j])
            for dl in (0, 1):
                GL = GLb + (int(Gh[f, MISSING_BIN]) if dl else 0)
                HL = HLb + (int(Hh[f, MISSING_BIN]) if dl else 0)
                GR, HR = Gp - GL, Hp - HL
                if HL <= 0 or HR <= 0:
                    continue
                if hess(HL) < mcw or hess(HR) < mcw:
                    continue
                if parent is None:
                    parent = gain(Gp, Hp, lam)          # (Hp = HL + HR > 0 here)
                loss = (gain(GL, HL, lam) + gain(GR, HR, lam)) - parent
                if best is None or loss > best[0]:
                    best = (loss, f, j, dl, GL, HL)
    return best


def grow_tree(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight):
    """grow_support.grow_tree with the fixed-point hessians hq uint64 [n]."""
    cut_ptr, cut_values = cuts
    F, n = bins.shape
    ncuts = [int(cut_ptr[f + 1]) - int(cut_ptr[f]) for f in range(F)]
    pos = np.zeros(n, dtype=np.int64)
    nodes = [dict(G=int(q.sum()), H=int(hq.astype(object).sum()), parent=-1)]
    level = [0]
    for d in range(max_depth):
        nxt = []
        for p in level:
            nd = nodes[p]
            rows = np.flatnonzero(pos == p)
            Gh = np.zeros((F, 256), dtype=np.int64)
            Hh = np.zeros((F, 256), dtype=np.uint64)
            for f in range(F):
                np.add.at(Gh[f], bins[f, rows], q[rows])
                np.add.at(Hh[f], bins[f, rows], hq[rows])
            best = best_split(Gh, Hh, ncuts, nd["G"], nd["H"], lam, min_child_weight)
            if best is None or not best[0] > float(np.float32(gamma)):
                continue
            loss, f, j, dl, GL, HL = best
            left = len(nodes)
            nd.update(left=left, right=left + 1, feature=f, j=j, dl=dl, loss=loss)
            nodes.append(dict(G=GL, H=HL, parent=p + G.LEFT_BIT))
            nodes.append(dict(G=nd["G"] - GL, H=nd["H"] - HL, parent=p))
            b = bins[f, rows]
            go_left = np.where(b == MISSING_BIN, bool(dl), b <= j)
            pos[rows] = np.where(go_left, left, left + 1)
            nxt += [left, left + 1]
        level = nxt
    m = len(nodes)
    t = {"left": np.full(m, -1, np.int32), "right": np.full(m, -1, np.int32), "parent": np.zeros(m, np.int32),
         "feature": np.zeros(m, np.uint32), "default_left": np.zeros(m, np.uint32), "value": np.zeros(m, np.float32),
         "loss_chg": np.zeros(m, np.float32), "sum_hess": np.zeros(m, np.float32), "base_weight": np.zeros(m, np.float32)}
    for i, nd in enumerate(nodes):
        leaf, w, sh = solve(nd["G"], nd["H"], eta, lam)
        t["parent"][i] = nd["parent"]
        t["sum_hess"][i] = sh
        t["base_weight"][i] = w
        if "left" in nd:
            t["left"][i], t["right"][i] = nd["left"], nd["right"]
            t["feature"][i], t["default_left"][i] = nd["feature"], nd["dl"]
            t["value"][i] = cut_values[int(cut_ptr[nd["feature"]]) + nd["j"]]
            t["loss_chg"][i] = np.float32(nd["loss"])
        else:
            t["value"][i] = leaf
    return t, pos


def weighted_sum(g, hq):
    """(S, W) as Python ints: S = sum hq * e^2 with e = rint(g * 2^24)."""
    scaled = np.asarray(g, dtype=np.float32) * R.SCALE
    assert scaled.dtype == np.float32
    e = np.rint(scaled).astype(np.int64)
    eo, ho = e.astype(object), np.asarray(hq).astype(object)      # Python ints: exact
    return int((ho * eo * eo).sum()) if len(eo) else 0, int(ho.sum()) if len(ho) else 0


def parts(g, hq):
    """(P2, P1, P0) as the header's device accumulators make them."""
    scaled = np.asarray(g, dtype=np.float32) * R.SCALE
    e = np.rint(scaled).astype(np.int64)
    m = 0xFFFFFFFF
    P2 = P1 = P0 = 0
    for h, v in zip(hq, e):
        sq = int(v) * int(v)
        a, b = sq >> 32, sq & m
        h = int(h)
        P2 += (h * a) >> 32
        P1 += ((h * a) & m) + ((h * b) >> 32)
        P0 += (h * b) & m
    return P2, P1, P0


def rmse(S, W):
    return math.sqrt((float(S) * 2.0 ** -72) / (float(W) * 2.0 ** -24))


def boost_weighted(pred, x, missing, y, w, cuts, num_feature, eval_set=None, eval_pred=None, rounds=1, patience=0,
                   max_depth=6, eta=0.3, lam=1.0, gamma=0.0, min_child_weight=1.0):
    """pred / eval_pred: the float32 margins of the forest so far; w: float32 weights or None; eval_set = (rows, missing,
    labels, weights or None) or None.  -> the dict of grow_eval_support.boost_eval, with train_W, eval_W and preds (the training margin
    after 0, 1, ... trees).  Raises
    ValueError with "label", "eval label", "weight", "eval weight" or "sum to 0" where the call is refused."""
    pred = np.asarray(pred, dtype=np.float32).copy()
    y = np.asarray(y, dtype=np.float32)
    n = len(y)
    wt = np.ones(n, np.float32) if w is None else np.asarray(w, dtype=np.float32)
    bins = G.bin_rows(x, missing, cuts, num_feature)
    # the gradient is looked at before the weight
    g0 = residuals(pred, y)
    wt = check_weights(wt, "weight")
    hq = hess_fixed(wt)
    if eval_set is not None:
        ex, emissing, ey, ew = (tuple(eval_set) + (None,))[:4]
        ey = np.asarray(ey, dtype=np.float32)
        ewt = np.ones(len(ey), np.float32) if ew is None else np.asarray(ew, dtype=np.float32)
        epred = np.asarray(eval_pred, dtype=np.float32).copy()
        eg0 = residuals(epred, ey, "eval label")
        ewt = check_weights(ewt, "eval weight")
        ehq = hess_fixed(ewt)
        eS0, eW = weighted_sum(eg0, ehq)
        eval_sums = [eS0]
    else:
        assert patience == 0
        eval_sums, eW, epred = None, None, None
    S0, W = weighted_sum(g0, hq)
    train_sums = [S0]
    trees, preds, epreds = [], [pred.copy()], [epred.copy() if epred is not None else None]
    run, best = rounds, 0
    for r in range(rounds):
        g = residuals(pred, y)
        q = grad_fixed(g, wt)
        t, pos = grow_tree(bins, q, hq, cuts, max_depth, eta, lam, gamma, min_child_weight)
        pred = pred + t["value"][pos]
        assert pred.dtype == np.float32
        trees.append(t)
        preds.append(pred.copy())
        train_sums.append(weighted_sum(residuals(pred, y), hq)[0])
        if eval_set is not None:
            epred = epred + E.walk(t, ex, emissing)
            assert epred.dtype == np.float32
            epreds.append(epred.copy())
            eval_sums.append(weighted_sum(residuals(epred, ey, "eval label"), ehq)[0])
            if eval_sums[r + 1] < eval_sums[best]:
                best = r + 1
            if patience >= 1 and (r + 1) - best >= patience:
                run = r + 1
                break
    if W == 0:
        raise ValueError("the weights sum to 0")
    if eval_set is not None and eW == 0:
        raise ValueError("the eval weights sum to 0")
    if eval_set is None:
        best = run
    keep = best if patience >= 1 else rounds
    kept = trees[:keep]
    return {"trees": kept, "all_trees": trees, "train_sums": train_sums, "eval_sums": eval_sums, "train_W": W, "eval_W": eW,
            "train_rmse": [rmse(s, W) for s in train_sums],
            "eval_rmse": [rmse(s, eW) for s in eval_sums] if eval_sums is not None else None,
            "rounds_run": run, "best_round": best, "nodes_added": sum(len(t["left"]) for t in kept),
            "pred": preds[keep], "eval_pred": epreds[keep] if eval_set is not None else None, "preds": preds}
