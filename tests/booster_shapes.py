"""Adversarial 27-feature boosters and the rows that go with them (test support).

The synthetic OH boosters (synth.make_model) are nearly full down to their depth cap, every tree starts below the root
(phase 1), and a row seldom sits exactly on a threshold.  The boosters made here reach, on purpose, what the super-node
walkers (kernels.hip: walk_super, ring_walk_group, super_step_by_chain) treat as edges:
  * trees of both phases, chosen through the leaf covers that choose_super_phase (csrc/flatten.cpp) weighs;
  * root leaves, stumps, full trees of exactly 4 and exactly 5 super-node steps, lopsided chains down to depth 30 and
    random lopsided trees;
  * groups of four trees (the walkers' chains) that mix all of these, so that a group's trip count is its deepest
    tree's and the others walk on through fillers; last groups of 1 to 3 trees of unequal depth (the clamped duplicate
    chain);
  * thresholds from SPECIAL (+-0, denormals, +-3e38), from a normal distribution and from the rows themselves, each
    possibly moved to a float32 neighbour; random default directions.
Rows are random_rows plus "tie rows": rows led down a path of one of the booster's trees to an internal node whose
feature is then set AT its threshold or one float32 step either side - so that a < read as <=, or a feature one ulp
off, changes a leaf.  Tie rows hold no missing value: a wave made of them walks the kernels' missing-free form."""
import json

import numpy as np

from tests.test_random_forests import SPECIAL, random_rows, random_tree

NFEAT = 27
# what a booster of `make_booster` may hold per tree (the `kinds` argument)
KINDS = ("leaf", "stump", "small", "full4", "full5", "chain", "lopsided", "random")


class Tree:
    def __init__(self):
        self.left, self.right, self.feat, self.cond, self.dl, self.hess = [], [], [], [], [], []

    def node(self):
        for a, v in ((self.left, -1), (self.right, -1), (self.feat, 0), (self.cond, 0.0), (self.dl, 0), (self.hess, 1.0)):
            a.append(v)
        return len(self.left) - 1

    def split(self, n):
        l, r = self.node(), self.node()
        self.left[n], self.right[n] = l, r
        return l, r

    def depths(self):
        d = [0] * len(self.left)
        for n in range(len(self.left)):          # children are always numbered after their parent
            if self.left[n] != -1:
                d[self.left[n]] = d[self.right[n]] = d[n] + 1
        return d


def _shape(rng, kind):
    """The tree's structure (no thresholds yet)."""
    t = Tree()
    root = t.node()
    if kind == "leaf":
        return t
    if kind == "stump":
        t.split(root)
        return t
    if kind in ("full4", "full5", "small"):
        # a full tree of depth D: its leaves all have D's parity, which fixes its phase - odd D: phase 0, (D + 1) / 2
        # steps; even D: phase 1, D / 2 steps.  4 steps: depth 7 or 8; 5 steps: depth 9 or 10
        depth = {"full4": int(rng.choice([7, 8])), "full5": int(rng.choice([9, 10])),
                 "small": int(rng.integers(2, 7))}[kind]
        frontier = [root]
        for _ in range(depth):
            frontier = [c for n in frontier for c in t.split(n)]
        return t
    if kind == "chain":
        # one child a leaf at every level, the other goes on: depth 12 .. 30
        n = root
        for _ in range(int(rng.integers(12, 31))):
            l, r = t.split(n)
            n = l if rng.random() < 0.5 else r
        return t
    if kind == "lopsided":
        # a deep spine with short random side branches
        n = root
        for _ in range(int(rng.integers(14, 27))):
            l, r = t.split(n)
            n, side = (l, r) if rng.random() < 0.5 else (r, l)
            todo = [(side, 0)]
            while todo:
                m, d = todo.pop()
                if d < 3 and rng.random() < 0.6:
                    a, b = t.split(m)
                    todo += [(a, d + 1), (b, d + 1)]
        return t
    if kind == "random":
        left, right, _, _, _ = random_tree(rng, NFEAT, int(rng.integers(6, 13)), float(rng.uniform(0.2, 0.35)))
        t.left, t.right = list(left), list(right)
        n = len(left)
        t.feat, t.cond, t.dl, t.hess = [0] * n, [0.0] * n, [0] * n, [1.0] * n
        return t
    raise ValueError(kind)


def _force_phase(rng, t, phase):
    """Leaf covers that make choose_super_phase pick `phase` where the tree's leaf depths allow it: phase p pays for the
    leaves of depth parity p, so those get cover 1 and the others 1000."""
    d = t.depths()
    for n in range(len(t.left)):
        if t.left[n] == -1:
            t.hess[n] = 1.0 if (d[n] & 1) == phase else 1000.0
        else:
            t.hess[n] = float(rng.integers(1, 100))


class Thresholds:
    """Draws split conditions: SPECIAL, normal(0, 2) or a value of the feature in `rows` (finite ones), then one float32
    step down, none, or one step up."""

    def __init__(self, rng, rows=None, p_special=0.25, p_rows=0.45):
        self.rng, self.p_special, self.p_rows = rng, p_special, p_rows
        self.pool = None
        if rows is not None:
            self.pool = [np.unique(c[np.isfinite(c)]).astype(np.float32) for c in np.asarray(rows, dtype=np.float32).T]

    def base(self, f):
        u = self.rng.random()
        if self.pool is not None and u < self.p_rows and len(self.pool[f]):
            return np.float32(self.rng.choice(self.pool[f]))
        if u < self.p_rows + self.p_special:
            return np.float32(self.rng.choice(SPECIAL))
        return np.float32(self.rng.normal(0, 2))

    def __call__(self, f):
        return neighbour(self.rng, self.base(f))


def neighbour(rng, v):
    """v, or one float32 step below or above it (never to an infinity)."""
    k = rng.integers(0, 3)
    if k == 0:
        return np.float32(v)
    w = np.nextafter(np.float32(v), np.float32(np.inf if k == 2 else -np.inf))
    return np.float32(v) if np.isinf(w) else w


def make_tree(rng, kind, thresholds, phase=None, feature_weights=None):
    t = _shape(rng, kind)
    p = None if feature_weights is None else np.asarray(feature_weights, dtype=np.float64) / np.sum(feature_weights)
    for n in range(len(t.left)):
        if t.left[n] == -1:
            t.cond[n] = float(np.float32(rng.normal(0, 0.1)))
        else:
            t.feat[n] = int(rng.choice(NFEAT, p=p))
            t.cond[n] = float(thresholds(t.feat[n]))
            t.dl[n] = int(rng.integers(0, 2))
    _force_phase(rng, t, int(rng.integers(0, 2)) if phase is None else phase)
    return t


def booster_json(trees, base_score):
    docs = []
    for i, t in enumerate(trees):
        n = len(t.left)
        parents = [2147483647] * n
        for m in range(n):
            if t.left[m] != -1:
                parents[t.left[m]] = parents[t.right[m]] = m
        docs.append({"base_weights": [0.0] * n, "categories": [], "categories_nodes": [], "categories_segments": [],
                     "categories_sizes": [], "default_left": t.dl, "id": i, "left_children": t.left,
                     "loss_changes": [0.0] * n, "parents": parents, "right_children": t.right,
                     "split_conditions": t.cond, "split_indices": t.feat, "split_type": [0] * n, "sum_hessian": t.hess,
                     "tree_param": {"num_deleted": "0", "num_feature": str(NFEAT), "num_nodes": str(n),
                                    "size_leaf_vector": "0"}})
    doc = {"learner": {"attributes": {}, "feature_names": [], "feature_types": [],
                       "gradient_booster": {"model": {"gbtree_model_param": {"num_parallel_tree": "1",
                                                                             "num_trees": str(len(trees)),
                                                                             "size_leaf_vector": "0"},
                                                      "tree_info": [0] * len(trees), "trees": docs}, "name": "gbtree"},
                       "learner_model_param": {"base_score": "%.9g" % float(base_score), "num_class": "0",
                                               "num_feature": str(NFEAT), "num_target": "1"},
                       "objective": {"name": "reg:squarederror", "reg_loss_param": {"scale_pos_weight": "1"}}},
           "version": [1, 6, 0]}
    return json.dumps(doc).encode()


# Tree kinds by position for the small counts: the last group of 1 - 3 trees mixes depths (its missing chains repeat
# the last tree, whose walk is discarded); the first groups put a shallow tree in chain 0 beside deep ones.
SMALL_PLANS = {
    1: ["chain"],
    2: ["leaf", "full5"],
    3: ["stump", "chain", "full4"],
    5: ["leaf", "full5", "stump", "lopsided", "chain"],
    10: ["small", "full4", "chain", "leaf", "full5", "stump", "lopsided", "random", "leaf", "chain"],
}


def plan(rng, ntree):
    """Tree kinds for a booster of `ntree` trees: SMALL_PLANS, or every kind in shuffled groups behind two fixed ones
    (a root leaf / stump in chain 0 beside trees of 5 and more steps)."""
    if ntree in SMALL_PLANS:
        return list(SMALL_PLANS[ntree])
    kinds = ["leaf", "full5", "chain", "full4", "stump", "lopsided", "full5", "small"]
    while len(kinds) < ntree:
        kinds.append(str(rng.choice(KINDS, p=[0.12, 0.12, 0.12, 0.14, 0.14, 0.12, 0.12, 0.12])))
    return kinds[:ntree]


def make_booster(seed, ntree, rows=None, feature_weights=None):
    """-> (JSON image, [Tree]) of `ntree` trees of 27 features.  `rows`: where thresholds may come from."""
    rng = np.random.default_rng(seed)
    thresholds = Thresholds(rng, rows)
    trees = []
    for i, kind in enumerate(plan(rng, ntree)):
        phase = i & 1 if kind in ("chain", "lopsided", "random", "small") else None
        trees.append(make_tree(rng, kind, thresholds, phase, feature_weights))
    return booster_json(trees, np.float32(rng.normal(0, 1))), trees


def tie_rows(rng, trees, n, base=None):
    """n rows without missing values, each led down a random tree to a random internal node and set AT that node's
    threshold or one float32 step either side of it.  Where the path has constrained the node's feature so that the
    threshold is out of reach, the row keeps its value.  `base`: rows to start from (finite), else normal(0, 2)."""
    out = (rng.normal(0, 2, (n, NFEAT)).astype(np.float32) if base is None
           else base[rng.integers(0, len(base), n)].astype(np.float32))
    internal = [(ti, [m for m in range(len(t.left)) if t.left[m] != -1]) for ti, t in enumerate(trees)]
    internal = [x for x in internal if x[1]]
    parent_cache = {}
    for r in range(n):
        ti, nodes = internal[rng.integers(0, len(internal))]
        t = trees[ti]
        if ti not in parent_cache:
            par = {}
            for m in range(len(t.left)):
                if t.left[m] != -1:
                    par[t.left[m]] = (m, True)
                    par[t.right[m]] = (m, False)
            parent_cache[ti] = par
        par = parent_cache[ti]
        target = int(nodes[rng.integers(0, len(nodes))])
        # bounds per feature along the path: [lo, hi) as float32 values
        lo, hi = {}, {}
        m = target
        while m in par:
            p, is_left = par[m]
            f, c = t.feat[p], np.float32(t.cond[p])
            if is_left:
                hi[f] = min(hi.get(f, np.float32(np.inf)), c)
            else:
                lo[f] = max(lo.get(f, np.float32(-np.inf)), c)
            m = p
        for f in set(lo) | set(hi):
            a, b = lo.get(f, np.float32(-3e38)), hi.get(f, np.float32(3e38))
            if a < b:
                x = np.float32(float(a) + (float(b) - float(a)) * rng.random())
                out[r, f] = x if a <= x < b else a
        f = t.feat[target]
        v = neighbour(rng, np.float32(t.cond[target]))
        if lo.get(f, np.float32(-np.inf)) <= v < hi.get(f, np.float32(np.inf)):
            out[r, f] = v
    return out


def rows_for(seed, trees, n, missing, tie_fraction=0.5):
    """n rows for a booster: random_rows (NaN, -999.0, SPECIAL, ties among themselves) and, as the second part of the
    batch, tie rows (no missing values: the waves that hold only them walk the missing-free form).  For missing = +-inf
    both infinities are salted in (the marker is missing, the other one a value below / above every threshold)."""
    rng = np.random.default_rng(seed)
    ntie = int(n * tie_fraction)
    rows = random_rows(rng, n - ntie, NFEAT)
    if np.isinf(missing):
        salt = rng.random(rows.shape)
        rows[salt < 0.03] = np.float32(np.inf)
        rows[(salt >= 0.03) & (salt < 0.06)] = np.float32(-np.inf)
    if ntie:
        rows = np.concatenate([rows, tie_rows(rng, trees, ntie)])
    return np.ascontiguousarray(rows, dtype=np.float32)


# ---- the fused path: thresholds on the slab's engineered values ----

def engineered_rows(fields, k1, k2):
    """What the fields kernels feed the walk for levels k1..k2 (1-based): the compat mirror's gather (PL / 100 as a
    float32 division, 2-D fields broadcast over the levels), -999.0 and NaN included."""
    from oracle import xgb_oracle as O
    return O.gather_rows(fields, k1, k2)


def fields_booster(seed, ntree, rows, pl_feature=1):
    """A booster whose every threshold is a value the slab's rows hold for that feature, or one float32 step either
    side of it; PL (the engineered feature) splits a third of the nodes, every other root.  Any one-ulp error in an
    engineered value then flips the decision of the rows that hold it."""
    rng = np.random.default_rng(seed)
    thresholds = Thresholds(rng, rows, p_special=0.0, p_rows=1.0)
    w = np.ones(NFEAT)
    w[pl_feature] = (NFEAT - 1) / 2.0
    trees = []
    for i, kind in enumerate(plan(rng, ntree)):
        t = make_tree(rng, kind, thresholds, i & 1 if kind in ("chain", "lopsided", "random", "small") else None, w)
        if t.left[0] != -1 and i % 2 == 0:
            t.feat[0] = pl_feature
            t.cond[0] = float(thresholds(pl_feature))
        trees.append(t)
    return booster_json(trees, np.float32(rng.normal(0, 1))), trees


def thresholds_by_feature(trees):
    out = [set() for _ in range(NFEAT)]
    for t in trees:
        for n in range(len(t.left)):
            if t.left[n] != -1:
                out[t.feat[n]].add(float(np.float32(t.cond[n])))
    return out


# ---- feature contributions: consistent covers and long paths with repeated features ----

def _long_chain(rng, thresholds, distinct):
    """A chain of depth 30 whose features are `distinct` features, each at least once, with repeats: for 27, a
    permutation of all of them followed by 3 repeats; below 27, the distinct ones in random order with repeats
    scattered between them.  Its deepest paths are `distinct` features long and split on some feature again."""
    order = [int(f) for f in rng.permutation(NFEAT)[:distinct]]
    if distinct == NFEAT:
        seq = order + [int(f) for f in rng.choice(order, 30 - NFEAT)]
    else:
        seq = list(order)
        for _ in range(30 - distinct):
            k = int(rng.integers(1, len(seq)))
            seq.insert(k, seq[int(rng.integers(0, k))])     # a feature already on the path above
    t = Tree()
    n = t.node()
    for f in seq:
        l, r = t.split(n)
        t.feat[n], t.cond[n], t.dl[n] = f, float(thresholds(f)), int(rng.integers(0, 2))
        n = l if rng.random() < 0.5 else r
    for m in range(len(t.left)):
        if t.left[m] == -1:
            t.cond[m] = float(np.float32(rng.normal(0, 0.1)))
    _force_phase(rng, t, int(rng.integers(0, 2)))
    return t


def _consistent_covers(rng, t, zero_cover_leaves):
    """Leaves keep their 1 / 1000 covers (or get 0, never both children of one split), every split the sum of its
    children's: zero fractions from about 1e-3 to 1, and mean(root) == v({})."""
    if zero_cover_leaves:
        for n in range(len(t.left)):
            l, r = t.left[n], t.right[n]
            if l == -1:
                continue
            for c, sib in ((l, r), (r, l)):
                if t.left[c] == -1 and not (t.left[sib] == -1 and t.hess[sib] == 0.0) and rng.random() < 0.3:
                    t.hess[c] = 0.0
    for n in reversed(range(len(t.left))):          # children are always numbered after their parent
        if t.left[n] != -1:
            t.hess[n] = t.hess[t.left[n]] + t.hess[t.right[n]]


def contribs_booster(seed, ntree, zero_cover_leaves=False):
    """make_booster's shapes, thresholds and tie rows for feature contributions -> (JSON image, [Tree]).  Covers are
    consistent (_consistent_covers).  The first chain of the plan takes all 27 features and then repeats (a path in
    the 32-feature length class), the second 21 - 24 distinct features with repeats between them (the 24-feature
    class); the rest draw features uniformly, as make_booster does (about 18 distinct on a depth-30 chain).
    `zero_cover_leaves`: some leaves get cover 0 (a zero fraction of exactly 0; only leaves can - a split's cover
    must be > 0)."""
    rng = np.random.default_rng(seed)
    thresholds = Thresholds(rng)
    trees, chains = [], 0
    for i, kind in enumerate(plan(rng, ntree)):
        if kind == "chain" and chains < 2:
            t = _long_chain(rng, thresholds, NFEAT if chains == 0 else int(rng.integers(21, 25)))
            chains += 1
        else:
            t = make_tree(rng, kind, thresholds, i & 1 if kind in ("chain", "lopsided", "random", "small") else None)
        _consistent_covers(rng, t, zero_cover_leaves)
        trees.append(t)
    return booster_json(trees, np.float32(rng.normal(0, 1))), trees


def distinct_path_lengths(t):
    """(distinct features, whether some feature repeats) of every root-to-leaf path of a Tree below a split."""
    out = []

    def walk(n, feats):
        if t.left[n] == -1:
            if feats:
                out.append((len(set(feats)), len(set(feats)) < len(feats)))
            return
        walk(t.left[n], feats + [t.feat[n]])
        walk(t.right[n], feats + [t.feat[n]])
    walk(0, [])
    return out
