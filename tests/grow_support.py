"""Shared by the tree-growing tests: a numpy restatement of OHXBoosterBoostTrees and OHXQuantileCuts written from the
text of include/ohxgb.h alone, and what goes with it.  Nothing here calls the code under test.

Binning is np.searchsorted(side="right"); the histograms are np.add.at on int64; the prefix sums np.cumsum on int64; the
gains float64 in the stated order; the tie rule a plain ascending loop over (f, j, dl) with a strict >; the solve is
refit_support.solve."""
import json

import numpy as np

from tests import refit_support as R

MISSING_BIN = 255
ARRAYS = ("left", "right", "parent", "feature", "default_left", "value", "loss_chg", "sum_hess", "base_weight")
LEFT_BIT = -(1 << 31)


def quantile_cuts(x, missing, max_bins=255):
    """-> (cut_ptr uint64 [ncol + 1], cut_values float32), steps 1-5 of the header."""
    x = np.asarray(x, dtype=np.float32)
    ptr, vals = [0], []
    for c in range(x.shape[1]):
        v = x[:, c]
        keep = ~np.isnan(v) & np.isfinite(v)
        if not np.isnan(missing):
            keep &= v != np.float32(missing)
        s = np.sort(v[keep])
        u = np.unique(s)
        n, m = len(s), len(u)
        if m <= 1:
            cuts = []
        elif m <= max_bins:
            cuts = list(u[1:])
        else:
            cuts = []
            for j in range(1, max_bins):
                cand = s[(j * n) // max_bins]
                if cand == u[0] or (cuts and cand == cuts[-1]):
                    continue
                cuts.append(cand)
        vals += cuts
        ptr.append(len(vals))
    return np.asarray(ptr, dtype=np.uint64), np.asarray(vals, dtype=np.float32)


def bin_rows(x, missing, cuts, num_feature):
    """-> uint8 [num_feature][nrow]: b = #{j : c_j <= x}; NaN, `missing` or a column x lacks -> 255."""
    cut_ptr, cut_values = cuts
    x = np.asarray(x, dtype=np.float32)
    n, ncol = x.shape
    bins = np.full((num_feature, n), MISSING_BIN, dtype=np.uint8)
    for f in range(min(ncol, num_feature)):
        c = np.asarray(cut_values[int(cut_ptr[f]):int(cut_ptr[f + 1])], dtype=np.float32)
        v = x[:, f]
        miss = np.isnan(v)
        if not np.isnan(missing):
            miss |= v == np.float32(missing)
        b = np.searchsorted(c, np.where(miss, np.float32(0), v), side="right")
        bins[f] = np.where(miss, MISSING_BIN, b).astype(np.uint8)
    return bins


def gain(G, H, lam):
    Gd = np.float64(G) * 2.0 ** -24
    return (Gd * Gd) / (np.float64(H) + np.float64(np.float32(lam)))


def best_split(Gh, Hh, ncuts, Gp, Hp, lam, min_child_rows):
    """The split choice of one node: Gh int64 / Hh int64 [F][256].  -> None or (loss_chg float64, f, j, dl, GL, HL):
    ascending (f, j, dl), replaced only by a strictly larger loss_chg."""
    best = None
    parent = gain(Gp, Hp, lam)
    for f in range(Gh.shape[0]):
        nc = int(ncuts[f])
        if nc == 0:
            continue
        cg = np.cumsum(Gh[f, :nc], dtype=np.int64)
        ch = np.cumsum(Hh[f, :nc], dtype=np.int64)
        for j in range(nc):
            for dl in (0, 1):
                GL = int(cg[j]) + (int(Gh[f, MISSING_BIN]) if dl else 0)
                HL = int(ch[j]) + (int(Hh[f, MISSING_BIN]) if dl else 0)
                GR, HR = Gp - GL, Hp - HL
                if HL < min_child_rows or HR < min_child_rows:
                    continue
                loss = (gain(GL, HL, lam) + gain(GR, HR, lam)) - parent
                if best is None or loss > best[0]:
                    best = (loss, f, j, dl, GL, HL)
    return best


def grow_tree(bins, q, cuts, max_depth, eta, lam, gamma, min_child_rows):
    """One tree from the bins [F][n] and the fixed-point gradients q int64 [n] -> (dict of the nine node arrays,
    the node every row ends on)."""
    cut_ptr, cut_values = cuts
    F, n = bins.shape
    ncuts = [int(cut_ptr[f + 1]) - int(cut_ptr[f]) for f in range(F)]
    pos = np.zeros(n, dtype=np.int64)
    nodes = [dict(G=int(q.sum()), H=n, parent=-1)]
    level = [0]
    for d in range(max_depth):
        nxt = []
        for p in level:                                  # ascending id
            nd = nodes[p]
            if nd["H"] < 2 * min_child_rows:
                continue
            rows = np.flatnonzero(pos == p)
            Gh = np.zeros((F, 256), dtype=np.int64)
            Hh = np.zeros((F, 256), dtype=np.int64)
            for f in range(F):
                np.add.at(Gh[f], bins[f, rows], q[rows])
                np.add.at(Hh[f], bins[f, rows], 1)
            best = best_split(Gh, Hh, ncuts, nd["G"], nd["H"], lam, min_child_rows)
            if best is None or not best[0] > np.float64(np.float32(gamma)):
                continue
            loss, f, j, dl, GL, HL = best
            left = len(nodes)
            nd.update(left=left, right=left + 1, feature=f, j=j, dl=dl, loss=loss)
            nodes.append(dict(G=GL, H=HL, parent=p + LEFT_BIT))
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
        leaf, w = R.solve([nd["G"]], [nd["H"]], eta, lam)
        t["parent"][i] = nd["parent"]
        t["sum_hess"][i] = np.float32(nd["H"])
        t["base_weight"][i] = w[0]
        if "left" in nd:
            t["left"][i], t["right"][i] = nd["left"], nd["right"]
            t["feature"][i], t["default_left"][i] = nd["feature"], nd["dl"]
            t["value"][i] = cut_values[int(cut_ptr[nd["feature"]]) + nd["j"]]
            t["loss_chg"][i] = np.float32(nd["loss"])
        else:
            t["value"][i] = leaf[0]
    return t, pos


def boost(pred, x, missing, y, cuts, num_feature, rounds=1, max_depth=6, eta=0.3, lam=1.0, gamma=0.0,
          min_child_rows=1):
    """pred: the float32 margin of the forest so far.  -> dict: trees (a list of dicts of the nine arrays),
    nodes_added, pred (the running margin after the last round), preds (after every round).  Raises ValueError where
    the call is refused for a gradient out of range."""
    pred = np.asarray(pred, dtype=np.float32).copy()
    y = np.asarray(y, dtype=np.float32)
    bins = bin_rows(x, missing, cuts, num_feature)
    out = {"trees": [], "nodes_added": 0, "preds": []}
    for r in range(rounds):
        with np.errstate(invalid="ignore", over="ignore"):
            g = pred - y
        assert g.dtype == np.float32
        if not (np.all(np.isfinite(g)) and np.all(np.abs(g) < R.MAX_ABS_GRAD)):
            raise ValueError(f"round {r}: a gradient is not finite or reaches 256")
        scaled = g * R.SCALE
        assert scaled.dtype == np.float32
        q = np.rint(scaled).astype(np.int64)
        t, pos = grow_tree(bins, q, cuts, max_depth, eta, lam, gamma, min_child_rows)
        pred = pred + t["value"][pos]
        assert pred.dtype == np.float32
        out["trees"].append(t)
        out["nodes_added"] += len(t["left"])
        out["preds"].append(pred.copy())
    out["pred"] = pred
    return out


# ---- models ----

def tree_doc(t, tid, nfeat):
    """A restated tree as the JSON schema's tree object."""
    n = len(t["left"])
    par = [int(p) & 0x7FFFFFFF if p != -1 else 2147483647 for p in t["parent"]]
    return {"base_weights": [float(v) for v in t["base_weight"]], "categories": [], "categories_nodes": [],
            "categories_segments": [], "categories_sizes": [], "default_left": [int(v) for v in t["default_left"]],
            "id": tid, "left_children": [int(v) for v in t["left"]], "loss_changes": [float(v) for v in t["loss_chg"]],
            "parents": par, "right_children": [int(v) for v in t["right"]],
            "split_conditions": [float(v) for v in t["value"]], "split_indices": [int(v) for v in t["feature"]],
            "split_type": [0] * n, "sum_hessian": [float(v) for v in t["sum_hess"]],
            "tree_param": {"num_deleted": "0", "num_feature": str(nfeat), "num_nodes": str(n), "size_leaf_vector": "0"}}


def with_trees(image, trees):
    """The JSON model `image` with the restated trees appended."""
    doc = json.loads(bytes(image).decode())
    model = doc["learner"]["gradient_booster"]["model"]
    nfeat = int(doc["learner"]["learner_model_param"]["num_feature"])
    for t in trees:
        model["trees"].append(tree_doc(t, len(model["trees"]), nfeat))
        model["tree_info"].append(0)
    model["gbtree_model_param"]["num_trees"] = str(len(model["trees"]))
    return json.dumps(doc).encode()


def trees_of(image):
    """Every tree of a JSON model image as a dict of the nine arrays (parent in the file's JSON form: the plain id, root
    2147483647), whole numbers parsed as floats (a writer may print -0)."""
    doc = json.loads(bytes(image).decode(), parse_int=float)
    out = []
    for t in doc["learner"]["gradient_booster"]["model"]["trees"]:
        out.append({"left": np.asarray(t["left_children"], np.int32), "right": np.asarray(t["right_children"], np.int32),
                    "parent": np.asarray(t["parents"], np.int64), "feature": np.asarray(t["split_indices"], np.uint32),
                    "default_left": np.asarray(t["default_left"], np.uint32),
                    "value": np.asarray(t["split_conditions"], np.float32),
                    "loss_chg": np.asarray(t["loss_changes"], np.float32),
                    "sum_hess": np.asarray(t["sum_hessian"], np.float32),
                    "base_weight": np.asarray(t["base_weights"], np.float32)})
    return out


def same_tree(got, want):
    """got: a tree of trees_of; want: a restated tree.  -> the name of the first array that differs in a bit, or None.
    The JSON parent drops the left-child bit, which the children arrays pin: parent[left[i]] == parent[right[i]] == i."""
    for k in ARRAYS:
        a, b = got[k], want[k]
        if k == "parent":
            b = np.where(b == -1, 2147483647, b.astype(np.int64) & 0x7FFFFFFF)
            if not np.array_equal(a, b):
                return k
            continue
        if a.shape != b.shape:
            return k
        if a.dtype == np.float32:
            if not np.array_equal(a.view(np.uint32), np.asarray(b, np.float32).view(np.uint32)):
                return k
        elif not np.array_equal(a.astype(np.int64), np.asarray(b).astype(np.int64)):
            return k
    return None


def empty_model(nfeat, base=0.5):
    """A loaded model with 0 trees."""
    return R.stumps(0, nfeat=nfeat, base=base)
