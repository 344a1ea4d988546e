"""Shared by the leaf-refit tests: a numpy restatement of OHXBoosterRefitLeaves written from the text of
include/ohxgb.h alone, and what goes with it.  Nothing here calls the code under test.

The restatement loops over the trees.  Per tree: the leaf every row reaches (the walk below, or leaf ids handed in -
what XGBoosterPredict(option_mask = 16) returns), g = pred - y as a float32 array operation, q = np.rint on the float32
product g * 2^24 cast to int64, G by np.add.at on int64 and H by bincount, w in float64 rounded to float32 once,
new_leaf = w * eta as a float32 multiply, and pred += new_leaf[leaf] as a float32 array add."""
import json

import numpy as np

from tests import visits_support as V

SCALE = np.float32(2.0 ** 24)
MAX_ABS_GRAD = 256.0


def base_of(image):
    doc = json.loads(bytes(image).decode())
    assert doc["learner"]["objective"]["name"] in ("reg:squarederror", "reg:linear")
    return np.float32(float(doc["learner"]["learner_model_param"]["base_score"]))


def walk(tree, x, missing):
    """The file node of the leaf every row of x reaches: NaN, `missing` or a column x lacks takes the default child,
    v < cond goes left, +-inf is compared as the float it is."""
    x = np.asarray(x, dtype=np.float32)
    n, ncol = x.shape
    left = np.asarray(tree["left_children"], dtype=np.int64)
    right = np.asarray(tree["right_children"], dtype=np.int64)
    feat = np.asarray(tree["split_indices"], dtype=np.int64)
    cond = np.asarray(tree["split_conditions"], dtype=np.float32)
    dleft = np.asarray(tree["default_left"], dtype=bool)
    node = np.zeros(n, dtype=np.int64)
    rows = np.arange(n)
    while True:
        act = left[node] != -1
        if not act.any():
            return node
        r, m = rows[act], node[act]
        f = feat[m]
        v = np.full(len(r), np.nan, dtype=np.float32)
        has = f < ncol
        v[has] = x[r[has], f[has]]
        if not np.isnan(missing):
            v[v == np.float32(missing)] = np.nan
        with np.errstate(invalid="ignore"):
            go_left = np.where(np.isnan(v), dleft[m], v < cond[m])
        node[act] = np.where(go_left, left[m], right[m])


def leaf_nodes(tree):
    """The reachable leaves of a tree, in file node order: the library's dense leaf numbering."""
    return [n for n in sorted(V.reachable(tree)) if tree["left_children"][n] == -1]


def solve(G, H, eta, reg_lambda):
    """(new_leaf, w) float32 from int64 G and integer H > 0, element by element as the header writes it."""
    G = np.asarray(G, dtype=np.int64)
    H = np.asarray(H, dtype=np.uint64)
    w = (-(G.astype(np.float64) * 2.0 ** -24) / (H.astype(np.float64) + np.float64(np.float32(reg_lambda)))).astype(np.float32)
    leaf = w * np.float32(eta)
    assert leaf.dtype == np.float32
    return leaf, w


def refit(image, x, missing, y, eta=1.0, reg_lambda=1.0, unvisited=0, leaf_ids=None):
    """-> dict: value / base_weight (per tree float32 arrays over the file's nodes, as the forest holds them after the
    call), leaves_refit, pred (the float32 margin of the refit model, row by row), G / H (per tree, over the nodes) and
    max_abs_grad.  Raises ValueError where the call is refused for a gradient out of range."""
    trees = V.doc_trees(image)
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    assert y.shape == (len(x),)
    if leaf_ids is not None:
        leaf_ids = np.asarray(leaf_ids).reshape(len(x), len(trees))
    pred = np.full(len(x), base_of(image), dtype=np.float32)
    out = {"value": [], "base_weight": [], "G": [], "H": [], "leaves_refit": 0, "max_abs_grad": 0.0}
    for t, tree in enumerate(trees):
        ids = walk(tree, x, missing) if leaf_ids is None else leaf_ids[:, t].astype(np.int64)
        nnode = len(tree["left_children"])
        with np.errstate(invalid="ignore", over="ignore"):
            g = pred - y
        assert g.dtype == np.float32
        if not (np.all(np.isfinite(g)) and np.all(np.abs(g) < MAX_ABS_GRAD)):
            raise ValueError(f"tree {t}: a gradient is not finite or reaches 256")
        out["max_abs_grad"] = max(out["max_abs_grad"], float(np.abs(g).max()))
        scaled = g * SCALE
        assert scaled.dtype == np.float32
        q = np.rint(scaled).astype(np.int64)
        G = np.zeros(nnode, dtype=np.int64)
        np.add.at(G, ids, q)
        H = np.bincount(ids, minlength=nnode).astype(np.uint64)
        value = np.asarray(tree["split_conditions"], dtype=np.float32).copy()
        bw = np.asarray(tree["base_weights"], dtype=np.float32).copy()
        leaves = np.asarray(leaf_nodes(tree), dtype=np.int64)
        assert set(np.flatnonzero(H)) <= set(leaves.tolist())
        seen = leaves[H[leaves] > 0]
        value[seen], bw[seen] = solve(G[seen], H[seen], eta, reg_lambda)
        if unvisited:
            rest = leaves[H[leaves] == 0]
            value[rest] = np.float32(0.0)
            bw[rest] = np.float32(0.0)
        out["leaves_refit"] += len(seen)
        pred = pred + value[ids]
        assert pred.dtype == np.float32
        for k, v in (("value", value), ("base_weight", bw), ("G", G), ("H", H)):
            out[k].append(v)
    out["pred"] = pred
    return out


def leaf_tables(image, per_tree):
    """Per-tree node arrays -> one table in the library's dense leaf numbering."""
    return np.concatenate([np.asarray(a)[leaf_nodes(t)] for t, a in zip(V.doc_trees(image), per_tree)])


def with_leaves(image, value, base_weight):
    """The same JSON model with every tree's split_conditions and base_weights replaced (float32 arrays over the file's
    nodes: only leaves differ from the file's)."""
    doc = json.loads(bytes(image).decode())
    for tree, v, w in zip(doc["learner"]["gradient_booster"]["model"]["trees"], value, base_weight):
        assert len(v) == len(tree["split_conditions"]) == len(w)
        tree["split_conditions"] = [float(a) for a in np.asarray(v, dtype=np.float32)]
        tree["base_weights"] = [float(a) for a in np.asarray(w, dtype=np.float32)]
    return json.dumps(doc).encode()


def leaves_of(image):
    """(value, base_weight) per tree of a JSON model image, float32 over the file's nodes.  Whole numbers are parsed as
    floats: a writer may print negative zero as -0, which json would read as the integer 0."""
    doc = json.loads(bytes(image).decode(), parse_int=float)
    trees = doc["learner"]["gradient_booster"]["model"]["trees"]
    return ([np.asarray(t["split_conditions"], dtype=np.float32) for t in trees],
            [np.asarray(t["base_weights"], dtype=np.float32) for t in trees])


def stump(cond, feature=0, nfeat=3, base=0.5, leaves=(0.25, -0.5)):
    """One stump of `nfeat` features -> JSON image."""
    doc = json.loads(V.hand_booster()[0].decode())
    t = V._tree_doc(0, [1, -1, -1], [2, -1, -1], [feature, 0, 0], [float(np.float32(cond)), leaves[0], leaves[1]],
                    [2.0, 1.0, 1.0], nfeat)
    model = doc["learner"]["gradient_booster"]["model"]
    model["trees"], model["tree_info"] = [t], [0]
    model["gbtree_model_param"]["num_trees"] = "1"
    doc["learner"]["learner_model_param"]["num_feature"] = str(nfeat)
    doc["learner"]["learner_model_param"]["base_score"] = "%.9g" % float(np.float32(base))
    return json.dumps(doc).encode()


def stumps(ntree, nfeat=3, base=0.5):
    """`ntree` stumps (0 is allowed), tree t splitting feature t % nfeat at t / ntree - 0.5 -> JSON image."""
    doc = json.loads(V.hand_booster()[0].decode())
    model = doc["learner"]["gradient_booster"]["model"]
    model["trees"] = [V._tree_doc(t, [1, -1, -1], [2, -1, -1], [t % nfeat, 0, 0],
                                  [float(np.float32(t / ntree - 0.5)), 0.25, -0.5], [2.0, 1.0, 1.0], nfeat)
                      for t in range(ntree)]
    model["tree_info"] = [0] * ntree
    model["gbtree_model_param"]["num_trees"] = str(ntree)
    doc["learner"]["learner_model_param"]["num_feature"] = str(nfeat)
    doc["learner"]["learner_model_param"]["base_score"] = "%.9g" % float(np.float32(base))
    return json.dumps(doc).encode()


def stump_bound_ratio(image, x, y, got_value):
    """One stump refit with eta = 1, lambda = 0: the largest |leaf - m| / (2^-24 * (1 + |m|)) over its two leaves,
    m the float64 mean of -(base - y) over the leaf's rows computed from the float32 g.  The bound is derived: every
    q is within 2^-25 of g * 2^24 / 2^24, so the mean of the q is within 2^-25 of m; the one rounding to float32 adds at
    most 2^-24 |mean|."""
    tree = V.doc_trees(image)[0]
    ids = walk(tree, x, float("nan"))
    g = np.full(len(x), base_of(image), dtype=np.float32) - np.asarray(y, dtype=np.float32)
    worst = 0.0
    for n in leaf_nodes(tree):
        mine = ids == n
        if not mine.any():
            continue
        m = float(np.mean(-g[mine].astype(np.float64)))
        worst = max(worst, abs(float(got_value[n]) - m) / (2.0 ** -24 * (1.0 + abs(m))))
    return worst
