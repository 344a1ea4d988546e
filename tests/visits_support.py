"""Shared by the visit-count tests: the tests' own numpy restatement of what OHXBoosterGetVisitCounts returns and of
OHXBoosterRefreshCover's arithmetic, boosters of any feature count, and hand-made trees.

Nothing here calls the code under test.  Expected counts come from LEAF IDS (what XGBoosterPredict(option_mask = 16)
returns, a path already held to the CPU oracle): numpy bincount, then summed up the tree by `sum_up`."""
import json

import numpy as np

from tests import contribs_support as cs

DELETED = 4294967295


def doc_trees(image):
    """The trees of a JSON model image as dicts of python lists."""
    doc = json.loads(bytes(image).decode())
    return doc["learner"]["gradient_booster"]["model"]["trees"]


def reachable(tree):
    """Nodes reachable from the root, parents before children."""
    left, right = tree["left_children"], tree["right_children"]
    order = [0]
    for n in order:
        if left[n] != -1:
            order += [left[n], right[n]]
    return order


def sum_up(tree, leaf_counts):
    """Per-node counts of one tree from per-node counts that are set at the leaves only: a split is the sum of its two
    children, unreachable slots 0."""
    left, right = tree["left_children"], tree["right_children"]
    order = reachable(tree)
    out = np.zeros(len(left), dtype=np.uint64)
    for n in order:
        if left[n] == -1:
            out[n] = leaf_counts[n]
    for n in reversed(order):
        if left[n] != -1:
            out[n] = out[left[n]] + out[right[n]]
    return out


def expected_counts(trees, leaf_ids):
    """leaf_ids: (nrow, ntree) file node ids of the leaves the rows reach -> a list of per-node uint64 counts."""
    leaf_ids = np.asarray(leaf_ids).reshape(-1, len(trees))
    out = []
    for t, tree in enumerate(trees):
        ids = leaf_ids[:, t].astype(np.int64)
        assert np.array_equal(ids, leaf_ids[:, t]), "leaf ids are whole numbers"
        out.append(sum_up(tree, np.bincount(ids, minlength=len(tree["left_children"])).astype(np.uint64)))
    return out


def check_invariants(trees, counts, rows_seen):
    """A tree's root equals rows_seen, a split the sum of its children, unreachable and deleted slots are 0."""
    assert len(counts) == len(trees)
    for t, (tree, c) in enumerate(zip(trees, counts)):
        left, right = tree["left_children"], tree["right_children"]
        assert c.dtype == np.uint64 and len(c) == len(left), t
        assert int(c[0]) == rows_seen, (t, int(c[0]), rows_seen)
        seen = set(reachable(tree))
        for n in range(len(left)):
            if n not in seen:
                assert int(c[n]) == 0, (t, n)
            elif left[n] != -1:
                assert int(c[n]) == int(c[left[n]]) + int(c[right[n]]), (t, n)


def assert_same_counts(got, want, what=""):
    assert len(got) == len(want), what
    for t, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, t, np.flatnonzero(g != w)[:8])


def expected_cover(tree, counts, prior_weight):
    """float32(count) + prior_weight * sum_hess in float32, the product rounded and then the sum, for every reachable
    node; the others keep their value."""
    old = np.asarray(tree["sum_hessian"], dtype=np.float32)
    new = counts.astype(np.float32) + np.float32(prior_weight) * old      # two float32 array operations: two roundings
    assert new.dtype == np.float32
    out = old.copy()
    idx = np.asarray(reachable(tree), dtype=np.int64)
    out[idx] = new[idx]
    return out


def with_covers(image, covers):
    """The same JSON model with every tree's sum_hessian replaced."""
    doc = json.loads(bytes(image).decode())
    for tree, c in zip(doc["learner"]["gradient_booster"]["model"]["trees"], covers):
        assert len(c) == len(tree["sum_hessian"])
        tree["sum_hessian"] = [float(x) for x in np.asarray(c, dtype=np.float32)]
    return json.dumps(doc).encode()


def zero_count_splits(trees, counts):
    """(tree, node) of every reachable split no counted row passed, in file order."""
    return [(t, n) for t, (tree, c) in enumerate(zip(trees, counts)) for n in sorted(reachable(tree))
            if tree["left_children"][n] != -1 and int(c[n]) == 0]


def random_booster(seed, ntree, nfeat, max_depth=7, p_leaf=0.2):
    """A JSON booster of any feature count with consistent covers (tests/contribs_support.py) -> image bytes."""
    rng = np.random.default_rng(seed)
    return cs.random_booster(rng, ntree, nfeat, max_depth, p_leaf)[0]


def level_forest(seed, ntree, nfeat, depth=3):
    """Full trees of `depth` levels whose level d splits on feature (t + d) % nfeat everywhere: no feature repeats on a
    path, so no split is out of reach of a wide enough batch.  Consistent covers -> image bytes."""
    rng = np.random.default_rng(seed)
    shapes = []
    for t in range(ntree):
        left, right, feat, cond, dl = [-1], [-1], [0], [0.0], [0]
        frontier = [0]
        for d in range(depth):
            nxt = []
            for n in frontier:
                for side in (left, right):
                    for a, v in ((left, -1), (right, -1), (feat, 0), (cond, 0.0), (dl, 0)):
                        a.append(v)
                    side[n] = len(left) - 1
                    nxt.append(len(left) - 1)
                feat[n], cond[n], dl[n] = (t + d) % nfeat, float(np.float32(rng.normal(0, 0.7))), int(rng.integers(0, 2))
            frontier = nxt
        for n in frontier:
            cond[n] = float(np.float32(rng.normal(0, 0.1)))
        shapes.append((left, right, feat, cond, dl))
    return cs.booster_from_trees(rng, shapes, nfeat)[0]


def _tree_doc(i, left, right, feat, cond, hess, nfeat, deleted=()):
    n = len(left)
    parents = [2147483647] * n
    for m in range(n):
        if left[m] != -1:
            parents[left[m]] = parents[right[m]] = m
    sidx = [DELETED if m in deleted else feat[m] for m in range(n)]
    return {"base_weights": [0.0] * n, "categories": [], "categories_nodes": [], "categories_segments": [],
            "categories_sizes": [], "default_left": [0] * n, "id": i, "left_children": left, "loss_changes": [0.0] * n,
            "parents": parents, "right_children": right, "split_conditions": cond, "split_indices": sidx,
            "split_type": [0] * n, "sum_hessian": hess,
            "tree_param": {"num_deleted": str(len(deleted)), "num_feature": str(nfeat), "num_nodes": str(n),
                           "size_leaf_vector": "0"}}


def hand_booster():
    """Four hand-made trees of 3 features: a root leaf; a stump; a chain of three splits; a stump whose children sit in
    slots 3 and 4 behind two deleted slots -> (image bytes, leaf nodes per tree)."""
    nfeat = 3
    docs = [
        _tree_doc(0, [-1], [-1], [0], [0.25], [7.0], nfeat),
        _tree_doc(1, [1, -1, -1], [2, -1, -1], [0, 0, 0], [0.5, -1.0, 1.0], [5.0, 2.0, 3.0], nfeat),
        _tree_doc(2, [1, -1, 3, -1, 5, -1, -1], [2, -1, 4, -1, 6, -1, -1], [0, 0, 1, 0, 2, 0, 0],
                  [0.0, 0.1, 0.0, 0.2, 0.0, 0.3, 0.4], [10.0, 4.0, 6.0, 1.0, 5.0, 0.0, 5.0], nfeat),
        _tree_doc(3, [3, -1, -1, -1, -1], [4, -1, -1, -1, -1], [1, 0, 0, 0, 0], [0.5, 0.0, 0.0, -2.0, 2.0],
                  [9.0, 77.0, 88.0, 4.0, 5.0], nfeat, deleted=(1, 2)),
    ]
    doc = {"learner": {"attributes": {}, "feature_names": [], "feature_types": [],
                       "gradient_booster": {"model": {"gbtree_model_param": {"num_parallel_tree": "1", "num_trees": "4",
                                                                             "size_leaf_vector": "0"},
                                                      "tree_info": [0] * 4, "trees": docs}, "name": "gbtree"},
                       "learner_model_param": {"base_score": "0.5", "num_class": "0", "num_feature": str(nfeat),
                                               "num_target": "1"},
                       "objective": {"name": "reg:squarederror", "reg_loss_param": {"scale_pos_weight": "1"}}},
           "version": [1, 6, 0]}
    return json.dumps(doc).encode(), [[0], [1, 2], [1, 3, 5, 6], [3, 4]]
