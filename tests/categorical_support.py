"""Boosters with categorical splits, their rows and their checker (test support; docs/14_categorical.md).

* `make_booster`: a seeded JSON document in xgboost 1.6.0's schema whose trees (depth 1 to 18) mix numeric and categorical
  nodes.  Every categorical FEATURE has a largest category M from MAXES - inline sets (M < 32) and multi-word ones, both
  sides of every word edge - and every categorical node on it holds a set whose largest member is M.  Both default
  directions, a categorical root (tree 0) and a feature that is split numerically and categorically in one tree (tree 1).
* `predict`: the routing table of include/ohxgb.h restated in numpy - margins (float32, leaves added in tree order) and
  leaf ids.  Written from the table, not from the C++: it is the checker of categorical models, which the CPU oracle
  (oracle/) does not know and is never handed.
* `twin`: a booster whose every set is a suffix {k, ..., M} has a numeric twin (x < float(k) at the same nodes) that routes
  every row whose categorical columns lie in [0, M + 1) identically; the twin is a model the oracle reads.
  `assert_in_twin_range` keeps the rows inside that range."""
import json

import numpy as np

NFEAT = 27
MAXES = (0, 1, 30, 31, 32, 63, 64, 1000)


def capacity(m):
    """Bits of 1.6.0's per-node bit field for a set whose largest category is m."""
    return 32 * ((m + 1 + 31) // 32)


class Tree:
    def __init__(self):
        self.left, self.right, self.feat, self.cond, self.dl, self.stype = [], [], [], [], [], []
        self.cats = {}                         # node -> list of categories, in the order the file gives them

    def node(self):
        for a, v in ((self.left, -1), (self.right, -1), (self.feat, 0), (self.cond, 0.0), (self.dl, 0), (self.stype, 0)):
            a.append(v)
        return len(self.left) - 1

    def split(self, n):
        l, r = self.node(), self.node()
        self.left[n], self.right[n] = l, r
        return l, r

    def depth(self):
        d = [0] * len(self.left)
        for n in range(len(self.left)):
            if self.left[n] != -1:
                d[self.left[n]] = d[self.right[n]] = d[n] + 1
        return max(d)


def _grow(rng, depth, p_split, max_nodes=1500):
    """A tree of exactly `depth` levels below the root: one spine of that length, random branches beside it."""
    t = Tree()
    n = t.node()
    side = []
    for d in range(depth):
        l, r = t.split(n)
        n, other = (l, r) if rng.random() < 0.5 else (r, l)
        side.append((other, d + 1))
    while side and len(t.left) < max_nodes:
        m, d = side.pop()
        if d < depth and rng.random() < p_split:
            a, b = t.split(m)
            side += [(a, d + 1), (b, d + 1)]
    return t


def _set_for(rng, m, suffix):
    if suffix:
        return list(range(int(rng.integers(0, m + 1)), m + 1))
    members = [c for c in range(m) if rng.random() < (0.5 if m < 100 else 0.1)] + [m]
    rng.shuffle(members)                       # the file's order is not sorted: the reader must not rely on it
    return [int(c) for c in members]


def make_booster(seed, ntree, nfeat=NFEAT, maxes=MAXES, suffix=False, depths=None, p_cat=0.45, objective="reg:squarederror"):
    """-> (JSON image, [Tree], cat_max) where cat_max maps each categorical feature to its largest category M.
    Categorical features are the first len(maxes) odd features (1, 3, 5, ...): feature 2 q + 1 has M = maxes[q]."""
    rng = np.random.default_rng(seed)
    cat_max = {2 * q + 1: int(m) for q, m in enumerate(maxes)}
    assert max(cat_max) < nfeat
    cat_feats, num_feats = sorted(cat_max), [f for f in range(nfeat) if f not in cat_max]
    if depths is None:
        depths = [1, 2, 18] + [int(rng.integers(1, 19)) for _ in range(max(0, ntree - 3))]
    trees = []
    for ti in range(ntree):
        t = _grow(rng, depths[ti % len(depths)], float(rng.uniform(0.35, 0.6)))
        for n in range(len(t.left)):
            if t.left[n] == -1:
                t.cond[n] = float(np.float32(rng.normal(0, 0.1)))
                continue
            t.dl[n] = int(rng.integers(0, 2))
            is_cat = rng.random() < p_cat
            if ti == 0 and n == 0:
                is_cat = True                                      # a categorical root
            if ti == 1:
                is_cat = n == 0                                    # ... and one feature split both ways in a tree
            if is_cat:
                # every categorical feature in turn first, so that each M of `maxes` is met whatever the seed
                f = cat_feats[(ti + n) % len(cat_feats)] if n < 2 * len(cat_feats) else int(rng.choice(cat_feats))
                if ti == 1:
                    f = cat_feats[2 % len(cat_feats)]
                t.feat[n], t.stype[n] = f, 1
                t.cats[n] = _set_for(rng, cat_max[f], suffix)
                t.cond[n] = float("nan")                           # what a 1.6.0 writer puts there
            else:
                f = int(rng.choice(num_feats)) if ti != 1 else cat_feats[2 % len(cat_feats)]
                t.feat[n] = f
                hi = cat_max.get(f)
                t.cond[n] = float(np.float32(rng.normal(0, 1.5) if hi is None else rng.uniform(0, hi + 1)))
        trees.append(t)
    base = float(np.float32(rng.normal(0, 1)))
    return booster_json(trees, base, nfeat, cat_max, objective), trees, cat_max


def tree_doc(i, t, nfeat, as_twin=False):
    n = len(t.left)
    parents = [2147483647] * n
    for m in range(n):
        if t.left[m] != -1:
            parents[t.left[m]] = parents[t.right[m]] = m
    cond, stype = list(t.cond), list(t.stype)
    categories, nodes, segments, sizes = [], [], [], []
    for m in sorted(t.cats):
        if as_twin:
            s = sorted(t.cats[m])
            assert s == list(range(s[0], s[-1] + 1)), "the twin needs suffix sets"
            cond[m], stype[m] = float(s[0]), 0
        else:
            nodes.append(m)
            segments.append(len(categories))
            sizes.append(len(t.cats[m]))
            categories += t.cats[m]
    return {"base_weights": [0.0] * n, "categories": categories, "categories_nodes": nodes,
            "categories_segments": segments, "categories_sizes": sizes, "default_left": t.dl, "id": i,
            "left_children": t.left, "loss_changes": [0.0] * n, "parents": parents, "right_children": t.right,
            "split_conditions": cond, "split_indices": t.feat, "split_type": stype, "sum_hessian": [1.0] * n,
            "tree_param": {"num_deleted": "0", "num_feature": str(nfeat), "num_nodes": str(n), "size_leaf_vector": "0"}}


def booster_json(trees, base, nfeat, cat_max, objective="reg:squarederror", as_twin=False):
    names = [] if as_twin else ["f%d" % f for f in range(nfeat)]
    types = [] if as_twin else ["c" if f in cat_max else "float" for f in range(nfeat)]
    doc = {"learner": {"attributes": {}, "feature_names": names, "feature_types": types,
                       "gradient_booster": {"model": {"gbtree_model_param": {"num_parallel_tree": "1",
                                                                             "num_trees": str(len(trees)),
                                                                             "size_leaf_vector": "0"},
                                                      "tree_info": [0] * len(trees),
                                                      "trees": [tree_doc(i, t, nfeat, as_twin) for i, t in enumerate(trees)]},
                                            "name": "gbtree"},
                       "learner_model_param": {"base_score": "%.9g" % float(base), "num_class": "0",
                                               "num_feature": str(nfeat), "num_target": "1"},
                       "objective": {"name": objective, "reg_loss_param": {"scale_pos_weight": "1"}}},
           "version": [1, 6, 0]}
    return json.dumps(doc).encode()           # NaN is written as the token NaN, as xgboost writes it


def base_of(image):
    return np.float32(json.loads(image)["learner"]["learner_model_param"]["base_score"])


def twin(image, trees, cat_max, nfeat=NFEAT):
    """The numeric twin of a suffix-set booster: a model without categorical splits."""
    return booster_json(trees, base_of(image), nfeat, cat_max, as_twin=True)


def assert_in_twin_range(X, cat_max, missing):
    """Every value of a categorical column is missing or inside [0, M + 1): where twin and booster route alike."""
    X = np.asarray(X, dtype=np.float32)
    for f, m in cat_max.items():
        if f >= X.shape[1]:
            continue
        v = X[:, f]
        miss = np.isnan(v) | (v == np.float32(missing))
        bad = ~miss & ~((v >= 0) & (v < np.float32(m + 1)))
        assert not bad.any(), (f, m, v[bad][:5])


def rows(seed, n, cat_max, nfeat=NFEAT, missing=np.nan, p_missing=0.05, wild=True):
    """n rows: numeric columns normal(0, 1.5); categorical columns mostly whole categories of [0, M], some fractions
    inside [0, M + 1) and - `wild` - values outside it (negative, beyond the capacity, huge).  p_missing of the entries
    hold `missing` (or NaN where `missing` is finite, half of the time)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 1.5, (n, nfeat)).astype(np.float32)
    for f, m in cat_max.items():
        col = rng.integers(0, m + 1, n).astype(np.float32)
        frac = rng.random(n) < 0.2
        col[frac] = rng.uniform(0, m + 1, int(frac.sum())).astype(np.float32)
        col = np.minimum(col, np.nextafter(np.float32(m + 1), np.float32(0)))
        if wild:
            w = rng.random(n) < 0.1
            pool = np.array([-1, -0.5, -0.0, capacity(m) - 1, capacity(m), capacity(m) + 1, m + 0.999, 3e9, 1e30, -7,
                             m + 1, 2.7], dtype=np.float32)
            col[w] = rng.choice(pool, int(w.sum()))
        X[:, f] = col
    hole = rng.random((n, nfeat)) < p_missing
    if np.isnan(missing):
        X[hole] = np.nan
    else:
        X[hole] = np.where(rng.random(int(hole.sum())) < 0.5, np.float32(missing), np.float32(np.nan))
    return X


def edge_values(m, missing):
    size = capacity(m)
    return [-1.0, -0.5, -0.0, 0.0, float(m), m + 0.999, size - 1.0, float(size), size + 1.0, 2.7, 3e9, 1e30, float("nan"),
            float(missing)]


def edge_rows(seed, cat_max, nfeat=NFEAT, missing=np.nan, extra=()):
    """Rows that put every edge value (and `extra`) into each categorical column in turn, and into all of them at once."""
    rng = np.random.default_rng(seed)
    out = []
    base = rows(seed + 1, 8, cat_max, nfeat, missing, p_missing=0.0, wild=False)
    for q in range(len(edge_values(0, missing)) + len(extra)):
        for f, m in cat_max.items():
            vals = edge_values(m, missing) + list(extra)
            r = base[int(rng.integers(0, len(base)))].copy()
            r[f] = np.float32(vals[q])
            out.append(r)
        r = base[int(rng.integers(0, len(base)))].copy()
        for f, m in cat_max.items():
            r[f] = np.float32((edge_values(m, missing) + list(extra))[q])
        out.append(r)
    return np.array(out, dtype=np.float32)


# ---------------------------------------------------------------- the restatement

def walk(t, X, missing):
    """Leaf node id of every row, by the table of include/ohxgb.h: all rows step together, level by level."""
    n_rows, ncol = X.shape
    left, right = np.array(t.left), np.array(t.right)
    feat, dl = np.array(t.feat), np.array(t.dl, dtype=bool)
    is_cat = np.array(t.stype) == 1
    cond = np.array(t.cond, dtype=np.float32)
    size = np.zeros(len(left), dtype=np.float32)                     # Size = 32 * ceil((M + 1) / 32)
    for n, cats in t.cats.items():
        size[n] = capacity(max(cats))
    member = np.zeros((len(left), int(size.max()) if len(t.cats) else 1), dtype=bool)
    for n, cats in t.cats.items():
        member[n, cats] = True
    at = np.zeros(n_rows, dtype=np.int64)
    while True:
        idx = np.nonzero(left[at] != -1)[0]
        if len(idx) == 0:
            return at
        n = at[idx]
        f = feat[n]
        has = f < ncol                                               # a column the matrix lacks is missing
        v = np.where(has, X[idx, np.minimum(f, ncol - 1)], np.float32(np.nan)).astype(np.float32)
        miss = np.isnan(v) if np.isnan(missing) else (np.isnan(v) | (v == np.float32(missing)))
        with np.errstate(invalid="ignore"):
            num_left = v < cond[n]
            outside = (v < np.float32(0)) | (v >= size[n])           # compared as floats, before any cast
        category = is_cat[n] & ~miss & ~outside
        c = np.zeros(len(idx), dtype=np.int64)
        c[category] = np.trunc(v[category]).astype(np.int64)         # (int)v: 2.7 -> 2, -0.0 -> 0
        in_set = member[n, c] & category
        cat_left = np.where(outside, dl[n], ~in_set)                 # in the set -> RIGHT
        go_left = np.where(miss, dl[n], np.where(is_cat[n], cat_left, num_left))      # missing is tested FIRST
        at[idx] = np.where(go_left, left[n], right[n])


def predict(trees, base, X, missing=np.nan, ntree_limit=0):
    """-> (margins float32 [nrow], leaf ids float32 [nrow][L]) over trees [0, L), L = all trees for ntree_limit 0 or
    beyond the booster."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    L = len(trees) if ntree_limit == 0 or ntree_limit > len(trees) else ntree_limit
    acc = np.full(X.shape[0], np.float32(base), dtype=np.float32)
    leaves = np.zeros((X.shape[0], L), dtype=np.float32)
    for ti in range(L):
        at = walk(trees[ti], X, missing)
        acc = (acc + np.array(trees[ti].cond, dtype=np.float32)[at]).astype(np.float32)
        leaves[:, ti] = at
    return acc, leaves
