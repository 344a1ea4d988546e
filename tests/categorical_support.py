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
  `assert_in_twin_range` keeps the rows inside that range.
* `make_adversarial`, `walk_sparse`, `category_tie_rows`: named tree kinds and set kinds the first builder never makes
  (root leaves, depth-30 chains on one feature, several capacities on one path, repeated members, full sets, word-edge
  sets, the largest legal category), the restatement with a per-node sorted set instead of a dense table, and rows led
  to a node and set on an edge of its test."""
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


def predict(trees, base, X, missing=np.nan, ntree_limit=0, walker=None):
    """-> (margins float32 [nrow], leaf ids float32 [nrow][L]) over trees [0, L), L = all trees for ntree_limit 0 or
    beyond the booster.  `walker`: `walk` (the default) or `walk_sparse`."""
    walker = walker or walk
    X = np.ascontiguousarray(X, dtype=np.float32)
    L = len(trees) if ntree_limit == 0 or ntree_limit > len(trees) else ntree_limit
    acc = np.full(X.shape[0], np.float32(base), dtype=np.float32)
    leaves = np.zeros((X.shape[0], L), dtype=np.float32)
    for ti in range(L):
        at = walker(trees[ti], X, missing)
        acc = (acc + np.array(trees[ti].cond, dtype=np.float32)[at]).astype(np.float32)
        leaves[:, ti] = at
    return acc, leaves


# ---------------------------------------------------------------- the sparse restatement

def walk_sparse(t, X, missing):
    """`walk` with the set of every node kept as sorted (node, category) keys instead of a dense [node][Size] table -
    the only form a node of Size 2**24 allows.  The order of the tests is `walk`'s, line for line."""
    n_rows, ncol = X.shape
    left, right = np.array(t.left), np.array(t.right)
    feat, dl = np.array(t.feat), np.array(t.dl, dtype=bool)
    is_cat = np.array(t.stype) == 1
    cond = np.array(t.cond, dtype=np.float32)
    size = np.zeros(len(left), dtype=np.float32)                     # Size = 32 * ceil((M + 1) / 32)
    for n, cats in t.cats.items():
        size[n] = capacity(max(cats))
    keys = np.unique(np.array([(n << 25) | int(c) for n, cats in t.cats.items() for c in cats] + [-1], dtype=np.int64))
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
        key = (n << 25) | c
        pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
        in_set = (keys[pos] == key) & category
        cat_left = np.where(outside, dl[n], ~in_set)                 # in the set -> RIGHT
        go_left = np.where(miss, dl[n], np.where(is_cat[n], cat_left, num_left))      # missing is tested FIRST
        at[idx] = np.where(go_left, left[n], right[n])


# ---------------------------------------------------------------- adversarial boosters

MAX_CATEGORY = 2 ** 24 - 1                     # OHX_MAX_CATEGORY of include/ohxgb.h
KINDS = ("leaf", "cat_stump", "full_cat", "chain", "lopsided", "mixed_capacity")        # and "maxcat", on request
SET_KINDS = ("zero", "top", "full", "edges", "repeated", "random")                      # and "maxcat"
WORD_EDGES = (31, 32, 63, 64)
# capacities down a mixed_capacity spine: M < 32 above M >= 32 and the reverse, one word, two, three, 32
MIXED_MS = (20, 63, 31, 40, 5, 1000, 0, 64)
MIXED_FEATURE_M = 1000                         # the feature of MAXES whose nodes take them

# Tree kinds by position, as booster_shapes.SMALL_PLANS: "chain30" is a chain of exactly 30 levels.  The tile kernel
# walks trees (0, 1), (2, 3), ... side by side and an odd last one alone.
ADV_PLANS = {
    1: ["chain30"],
    2: ["leaf", "chain30"],
    3: ["chain30", "leaf", "mixed_capacity"],
    5: ["cat_stump", "full_cat", "leaf", "lopsided", "chain"],
    10: ["leaf", "chain30", "chain30", "leaf", "full_cat", "mixed_capacity", "cat_stump", "lopsided", "chain", "leaf"],
}


def adv_plan(rng, ntree):
    if ntree in ADV_PLANS:
        return list(ADV_PLANS[ntree])
    kinds = list(ADV_PLANS[10])
    while len(kinds) < ntree:
        kinds.append(str(rng.choice(KINDS)))
    return kinds[:ntree]


def adv_set(rng, kind, m):
    """-> the member list of a set of `kind` whose node is meant for a feature of largest category m (the list's own
    largest member, which fixes the node's capacity, is 0 for "zero" and 2**24 - 1 for "maxcat")."""
    if kind == "zero":
        return [0]
    if kind == "top":
        return [int(m)]
    if kind == "full":
        return list(range(int(m) + 1))
    if kind == "edges":
        assert m in WORD_EDGES
        return [int(c) for c in reversed(WORD_EDGES) if c <= m]
    if kind == "repeated":
        members = [int(c) for c in range(m) if rng.random() < (0.4 if m < 100 else 0.05)] + [int(m)]
        members += [int(c) for c in rng.choice(members, len(members) // 2 + 2)]      # again, anywhere in the list
        rng.shuffle(members)
        return [int(c) for c in members]
    if kind == "random":
        return _set_for(rng, m, False)
    if kind == "maxcat":
        return [40, MAX_CATEGORY, 0, 3]
    raise ValueError(kind)


def neighbour(rng, v):
    """v, or one float32 step below or above it."""
    k = int(rng.integers(0, 3))
    if k == 0:
        return np.float32(v)
    return np.nextafter(np.float32(v), np.float32(np.inf if k == 2 else -np.inf))


class _Adv:
    """What make_adversarial draws from: set kinds in turn (every kind comes up whatever the seed), features by M."""

    def __init__(self, rng, nfeat, maxes):
        self.rng = rng
        self.cat_max = {2 * q + 1: int(m) for q, m in enumerate(maxes)}
        self.cat_feats = sorted(self.cat_max)
        self.num_feats = [f for f in range(nfeat) if f not in self.cat_max]
        self.turn = 0

    def cat_node(self, t, n, f=None, kind=None, m=None):
        rng = self.rng
        if kind is None:
            kind = SET_KINDS[self.turn % len(SET_KINDS)]
            self.turn += 1
        if f is None:
            pool = [g for g in self.cat_feats if kind != "edges" or self.cat_max[g] in WORD_EDGES]
            f = pool[int(rng.integers(0, len(pool)))]
            if kind == "edges" and self.turn <= len(SET_KINDS):
                f = [g for g in pool if self.cat_max[g] == 64][0]              # all four edges at least once
        if m is None:
            m = self.cat_max[f]
        if kind == "edges" and m not in WORD_EDGES:
            kind = "top"
        t.feat[n], t.stype[n], t.cond[n], t.dl[n] = f, 1, float("nan"), int(rng.integers(0, 2))
        t.cats[n] = adv_set(rng, kind, m)
        t.setkind[n] = kind

    def num_node(self, t, n, f=None):
        rng = self.rng
        if f is None:
            f = int(rng.choice(self.num_feats)) if rng.random() < 0.6 else int(rng.choice(self.cat_feats))
        t.feat[n], t.dl[n] = f, int(rng.integers(0, 2))
        if f in self.cat_max:
            # on a categorical column: at an integer of [0, M + 1] or a float32 neighbour of it
            t.cond[n] = float(neighbour(rng, np.float32(rng.integers(0, self.cat_max[f] + 2))))
        else:
            t.cond[n] = float(neighbour(rng, np.float32(rng.normal(0, 1.5))))

    def any_node(self, t, n):
        if self.rng.random() < 0.5:
            self.cat_node(t, n)
        else:
            self.num_node(t, n)


def _adv_tree(a, kind):
    rng = a.rng
    t = Tree()
    t.setkind = {}
    t.witness = {}                              # feature -> a value that reaches the deepest node of a spine
    t.kind = "chain" if kind == "chain30" else kind
    root = t.node()
    if kind == "leaf":
        pass
    elif kind == "cat_stump":
        t.split(root)
        a.cat_node(t, root)
    elif kind == "full_cat":
        frontier = [root]
        for _ in range(int(rng.integers(3, 6))):
            nxt = []
            for n in frontier:
                nxt += t.split(n)
                a.cat_node(t, n)
            frontier = nxt
    elif kind in ("chain", "chain30"):
        # numeric and categorical splits in turn, all on ONE categorical feature
        f = [g for g in a.cat_feats if a.cat_max[g] >= 63][int(rng.integers(0, 3))]
        # the chain goes on where the witness value goes, so that its last level can be reached at all
        t.witness[f] = np.float32(rng.integers(0, a.cat_max[f] + 1)) + np.float32(rng.choice([0.0, 0.5]))
        n = root
        for d in range(30 if kind == "chain30" else int(rng.integers(12, 31))):
            l, r = t.split(n)
            if d & 1:
                a.cat_node(t, n, f=f, kind=str(rng.choice(["random", "repeated", "top", "full", "zero"])))
            else:
                a.num_node(t, n, f=f)
            n = l if goes_left(t, n, t.witness[f]) else r
    elif kind == "lopsided":
        n = root
        for _ in range(int(rng.integers(14, 27))):
            l, r = t.split(n)
            a.any_node(t, n)
            n, side = (l, r) if rng.random() < 0.5 else (r, l)
            todo = [(side, 0)]
            while todo:
                m, d = todo.pop()
                if d < 3 and rng.random() < 0.6:
                    x, y = t.split(m)
                    a.any_node(t, m)
                    todo += [(x, d + 1), (y, d + 1)]
    elif kind == "mixed_capacity":
        # one feature, categorical at every node of a spine, a different capacity at each
        f = [g for g in a.cat_feats if a.cat_max[g] == MIXED_FEATURE_M][0]
        # 40: a category at the nodes of M >= 40, outside at those below (the default child)
        t.witness[f] = np.float32(40.0)
        n = root
        for m in MIXED_MS:
            l, r = t.split(n)
            a.cat_node(t, n, f=f, kind="zero" if m == 0 else str(rng.choice(["random", "top", "repeated"])), m=m)
            n = l if goes_left(t, n, t.witness[f]) else r
    elif kind == "maxcat":
        # the largest legal category: 524 288 set words, Size = 2**24; a numeric split of the same column below it
        f = a.cat_feats[0]
        l, r = t.split(root)
        a.cat_node(t, root, f=f, kind="maxcat")
        t.split(l)
        t.feat[l], t.dl[l], t.cond[l] = f, int(rng.integers(0, 2)), 8388608.0
    else:
        raise ValueError(kind)
    for n in range(len(t.left)):
        if t.left[n] == -1:
            t.cond[n] = float(np.float32(rng.normal(0, 0.1)))
    return t


def make_adversarial(seed, ntree, nfeat=NFEAT, maxes=MAXES, maxcat=False, kinds=None):
    """-> (JSON image, [Tree], cat_max).  Trees carry `.kind` and `.setkind` (node -> kind of its set).  `kinds`: the
    tree kinds by position, else adv_plan's; `maxcat` makes the LAST tree the one with category 2**24 - 1 (on feature 1,
    whose cat_max then is that category)."""
    rng = np.random.default_rng(seed)
    a = _Adv(rng, nfeat, maxes)
    assert max(a.cat_max) < nfeat
    kinds = list(kinds) if kinds is not None else adv_plan(rng, ntree)
    assert len(kinds) == ntree
    if maxcat:
        kinds[-1] = "maxcat"
    trees = [_adv_tree(a, k) for k in kinds]
    cat_max = dict(a.cat_max)
    for t in trees:
        for n, cats in t.cats.items():
            cat_max[t.feat[n]] = max(cat_max[t.feat[n]], max(cats))
    base = float(np.float32(rng.normal(0, 1)))
    return booster_json(trees, base, nfeat, cat_max), trees, cat_max


# ---------------------------------------------------------------- tie rows

DENORMAL = np.float32(2.0 ** -149)


def goes_left(t, n, v):
    """The routing table for ONE value that is not missing."""
    v = np.float32(v)
    if t.stype[n] == 1:
        if v < np.float32(0) or v >= np.float32(capacity(max(t.cats[n]))):
            return bool(t.dl[n])
        return int(v) not in t.cats[n]
    return bool(v < np.float32(t.cond[n]))


def edge_candidates(rng, t, n):
    """The values of category_tie_rows for node n, as float32."""
    if t.stype[n] != 1:
        c = np.float32(t.cond[n])
        return [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    cats = t.cats[n]
    size = np.float32(capacity(max(cats)))
    some = [cats[int(i)] for i in rng.integers(0, len(cats), 4)] + [max(cats), min(cats)]
    out = []
    for c in some:
        out += [c, c - 1, c + 1, np.nextafter(np.float32(c), np.float32(0)), np.nextafter(np.float32(c + 1), np.float32(0))]
    out += [size - np.float32(1), np.nextafter(size, np.float32(0)), size, np.float32(-0.0), DENORMAL, -DENORMAL]
    return [np.float32(x) for x in out]


def category_tie_rows(rng, trees, n, cat_max, nfeat=NFEAT):
    """n rows without a missing value, each led down a random tree to a random internal node.  At a categorical node
    the row then holds a member, a member - 1 or + 1, the float32 just below an integer (it truncates to the category
    below), Size - 1, nextafter(Size, 0), Size, -0.0 or the smallest denormal of either sign; at a numeric node the
    threshold or a float32 neighbour.  Of those, one that the path to the node allows (the path may test the same
    feature many times: every candidate is tried against all of them); where none does, a value the path allows."""
    out = rows(int(rng.integers(0, 2 ** 31)), n, cat_max, nfeat, np.nan, p_missing=0.0, wild=False)
    internal = [(t, [m for m in range(len(t.left)) if t.left[m] != -1]) for t in trees]
    internal = [x for x in internal if x[1]]
    parents = {}
    for r in range(n):
        t, nodes = internal[int(rng.integers(0, len(internal)))]
        if id(t) not in parents:
            parents[id(t)] = {c: (m, side) for m in range(len(t.left)) if t.left[m] != -1
                              for c, side in ((t.left[m], True), (t.right[m], False))}
        par = parents[id(t)]
        target = int(nodes[int(rng.integers(0, len(nodes)))])
        path = {}                                                    # feature -> [(node, went left)]
        m = target
        while m in par:
            p, is_left = par[m]
            path.setdefault(t.feat[p], []).append((p, is_left))
            m = p

        def allowed(f, v):
            return all(goes_left(t, p, v) == side for p, side in path.get(f, []))

        for f, steps in path.items():
            if allowed(f, out[r, f]):
                continue
            cands = [v for p, _ in steps for v in edge_candidates(rng, t, p)]
            cands += [np.float32(x) for x in rng.integers(0, cat_max.get(f, 64) + 40, 40)] + [np.float32(-1)]
            cands += [t.witness[f]] if f in getattr(t, "witness", {}) else []
            good = [v for v in cands if allowed(f, v)]
            if good:
                out[r, f] = good[int(rng.integers(0, len(good)))]
        f = t.feat[target]
        good = [v for v in edge_candidates(rng, t, target) if allowed(f, v)]
        if good:
            out[r, f] = good[int(rng.integers(0, len(good)))]
    assert not np.isnan(out).any()
    return out
