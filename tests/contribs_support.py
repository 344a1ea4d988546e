"""Shared by the contribution tests: random boosters with consistent cover statistics, and a float64 brute-force
Shapley reference.

The value function of a tree (path-dependent TreeSHAP's):
    v(S) = sum over leaves of value * prod over the path's splits of
           [feature in S ? 1{x takes this child} : cover(child) / cover(parent)]
phi_i = sum over S in F minus {i} of |S|! (M - |S| - 1)! / M! * (v(S + i) - v(S)); the bias is v({}) + the margin base.
"""
import json
import math

import numpy as np

from tests.test_random_forests import random_tree, random_rows  # noqa: F401  (random_rows re-exported)


def with_covers(rng, left, right, zero_leaves=0.0):
    """Leaves get a random integer cover, a split the sum of its children's: then mean(root) == v({}).  With
    probability `zero_leaves` a leaf gets cover 0 instead, unless its sibling is a leaf of cover 0 (a split's cover
    must stay > 0)."""
    n = len(left)
    cover = [0.0] * n
    zero = set()
    for i in range(n):
        if left[i] != -1:
            for c, sib in ((left[i], right[i]), (right[i], left[i])):
                if left[c] == -1 and sib not in zero and rng.random() < zero_leaves:
                    zero.add(c)

    def fill(i):
        if left[i] == -1:
            cover[i] = 0.0 if i in zero else float(rng.integers(1, 50))
        else:
            cover[i] = fill(left[i]) + fill(right[i])
        return cover[i]
    fill(0)
    return cover


def random_booster(rng, ntree, nfeat, max_depth, p_leaf, base_score=None, zero_leaves=0.0):
    """(json bytes, trees, base) - trees as dicts of python lists, for the brute force."""
    return booster_from_trees(rng, [random_tree(rng, nfeat, max_depth, p_leaf) for _ in range(ntree)], nfeat,
                              base_score, zero_leaves)


def caterpillar_tree(rng, nfeat, length):
    """A chain of `length` splits on distinct features, a leaf beside every split: paths of every length 1..length."""
    left, right, feat, cond, dl = [], [], [], [], []

    def new():
        left.append(-1); right.append(-1); feat.append(0); cond.append(float(np.float32(rng.normal(0, 0.1))))
        dl.append(0)
        return len(left) - 1
    order = rng.permutation(nfeat)[:length]
    n = new()
    for f in order:
        l, r = new(), new()
        left[n], right[n] = l, r
        feat[n] = int(f)
        cond[n] = float(np.float32(rng.normal(0, 1.0)))
        dl[n] = int(rng.integers(0, 2))
        n = l if rng.random() < 0.5 else r
    return left, right, feat, cond, dl


def caterpillar_booster(rng, ntree, nfeat, length):
    return booster_from_trees(rng, [caterpillar_tree(rng, nfeat, length) for _ in range(ntree)], nfeat)


def booster_from_trees(rng, shapes, nfeat, base_score=None, zero_leaves=0.0):
    ntree = len(shapes)
    trees, docs = [], []
    for t, (left, right, feat, cond, dl) in enumerate(shapes):
        cover = with_covers(rng, left, right, zero_leaves)
        n = len(left)
        parents = [2147483647] * n
        for i in range(n):
            if left[i] != -1:
                parents[left[i]] = i
                parents[right[i]] = i
        trees.append({"left": left, "right": right, "feat": feat, "cond": cond, "dl": dl, "cover": cover})
        docs.append({"base_weights": [0.0] * n, "categories": [], "categories_nodes": [], "categories_segments": [],
                     "categories_sizes": [], "default_left": dl, "id": t, "left_children": left,
                     "loss_changes": [0.0] * n, "parents": parents, "right_children": right,
                     "split_conditions": cond, "split_indices": feat, "split_type": [0] * n,
                     "sum_hessian": cover,
                     "tree_param": {"num_deleted": "0", "num_feature": str(nfeat), "num_nodes": str(n),
                                    "size_leaf_vector": "0"}})
    if base_score is None:
        base_score = float(np.float32(rng.normal(0, 1)))
    doc = {"learner": {"attributes": {}, "feature_names": [], "feature_types": [],
                       "gradient_booster": {"model": {"gbtree_model_param": {"num_parallel_tree": "1",
                                                                             "num_trees": str(ntree),
                                                                             "size_leaf_vector": "0"},
                                                      "tree_info": [0] * ntree, "trees": docs}, "name": "gbtree"},
                       "learner_model_param": {"base_score": "%.9g" % base_score, "num_class": "0",
                                               "num_feature": str(nfeat), "num_target": "1"},
                       "objective": {"name": "reg:squarederror", "reg_loss_param": {"scale_pos_weight": "1"}}},
           "version": [1, 6, 0]}
    return json.dumps(doc).encode(), trees, float(np.float32(base_score))


def _tree_values(tree, x, missing, nfeat):
    """v(S) of one tree for every subset S (bit j of the index = feature j in S), float64."""
    masks = np.arange(1 << nfeat)

    def is_missing(f):
        if f >= len(x):
            return True
        v = x[f]
        return np.isnan(v) or (not np.isnan(missing) and v == missing)

    def val(n):
        if tree["left"][n] == -1:
            return np.full(masks.shape, float(np.float32(tree["cond"][n])))
        f = tree["feat"][n]
        l, r = tree["left"][n], tree["right"][n]
        if is_missing(f):
            hot = l if tree["dl"][n] else r
        else:
            hot = l if np.float32(x[f]) < np.float32(tree["cond"][n]) else r
        vl, vr = val(l), val(r)
        cov = tree["cover"][n]
        expect = tree["cover"][l] / cov * vl + tree["cover"][r] / cov * vr
        return np.where((masks >> f) & 1, vl if hot == l else vr, expect)
    return val(0)


def brute_force(trees, base, rows, missing, nfeat, ntree_limit=0):
    """(nrow, nfeat + 1) float64 Shapley values of the booster's margin."""
    use = trees[:ntree_limit] if ntree_limit else trees
    M = nfeat
    masks = np.arange(1 << M)
    size = np.array([bin(m).count("1") for m in masks])
    weight = np.array([math.factorial(s) * math.factorial(M - s - 1) / math.factorial(M) if s < M else 0.0
                       for s in size])
    out = np.zeros((len(rows), M + 1))
    for r, x in enumerate(rows):
        V = np.zeros(1 << M)
        for t in use:
            V += _tree_values(t, x, missing, nfeat)
        for i in range(M):
            without = masks[((masks >> i) & 1) == 0]
            out[r, i] = np.sum(weight[without] * (V[without | (1 << i)] - V[without]))
        out[r, M] = V[0] + base
    return out


def _paths_of(t):
    """Every leaf below a split: its distinct features with interval, missing bit and merged zero fraction."""
    out=[]
    def walk(n, path):
        if t["left"][n]==-1:
            if path: out.append(([dict(e) for e in path], t["cond"][n]))
            return
        f=t["feat"][n]; c=np.float32(t["cond"][n]); cov=t["cover"][n]
        for side,ch in ((0,t["left"][n]),(1,t["right"][n])):
            miss = (bool(t["dl"][n]) == (side==0))
            z=t["cover"][ch]/cov
            old=[dict(e) for e in path]
            k=next((i for i,e in enumerate(path) if e["f"]==f),None)
            if k is None: path.append({"f":f,"lo":None,"hi":None,"m":True,"z":1.0}); k=len(path)-1
            e=path[k]
            if side==0: e["hi"]=c if e["hi"] is None else min(e["hi"],c)
            else: e["lo"]=c if e["lo"] is None else max(e["lo"],c)
            e["m"]=e["m"] and miss; e["z"]*=z
            walk(ch,path)
            path[:]=old
    walk(0,[])
    return out

def tree_dicts(trees):
    """tests/booster_shapes.py Trees as the dicts of python lists the references here take."""
    return [{"left": t.left, "right": t.right, "feat": t.feat, "cond": t.cond, "dl": t.dl, "cover": t.hess}
            for t in trees]


def _full_width(rows, nfeat):
    """rows with the columns the matrix does not have added as NaN: they are missing."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.shape[1] < nfeat:
        rows = np.concatenate([rows, np.full((len(rows), nfeat - rows.shape[1]), np.nan, np.float32)], axis=1)
    return rows


def treeshap64(trees, base, rows, missing, nfeat, chunk=2048):
    """Path-dependent TreeSHAP in float64, path by path as the kernels evaluate it (one element per distinct feature,
    intervals, merged zero fractions) - exact to float64 rounding, so a reference where the brute force cannot go
    (more than 10 features); checked against the brute force in test_contribs_cpu.py.  Columns the matrix does not
    have are missing.  Paths of one length run together, `chunk` at a time.  An element with z = 0 and o = 0 (a leaf
    of cover 0 the row does not reach) adds nothing: its unwound term is never divided by z, and its share is
    multiplied by o - z = 0."""
    dt = np.float64
    rows = _full_width(rows, nfeat)
    n = len(rows)
    out = np.zeros((n, nfeat + 1), dt)
    miss_all = np.isnan(rows) | (rows == missing)
    by_len = {}
    for t in trees:
        for path, v in _paths_of(t):
            by_len.setdefault(len(path), []).append((path, v))
        out[:, nfeat] += _mean_root(t)
    phi = np.zeros((nfeat, n), dt)
    for d, paths in sorted(by_len.items()):
        for c0 in range(0, len(paths), chunk):
            part = paths[c0:c0 + chunk]
            feat = np.array([[e["f"] for e in p] for p, _ in part])
            # an open end (None -> NaN) holds every value, +-inf included
            lo = np.array([[np.nan if e["lo"] is None else e["lo"] for e in p] for p, _ in part], np.float32)
            hi = np.array([[np.nan if e["hi"] is None else e["hi"] for e in p] for p, _ in part], np.float32)
            bit = np.array([[e["m"] for e in p] for p, _ in part])
            Z = np.array([[e["z"] for e in p] for p, _ in part], dt)
            leaf = np.array([np.float32(v) for _, v in part], dt)
            x = rows.T[feat]                                   # (paths, d, n)
            inside = ~(x < lo[..., None]) & ~(x >= hi[..., None])
            O = np.where(miss_all.T[feat], bit[..., None], inside).astype(dt)
            pw = np.zeros((d + 1,) + O[:, 0].shape, dt)
            pw[0] = 1
            for k in range(1, d + 1):
                z = Z[:, k - 1, None]; of = O[:, k - 1]
                for i in range(k - 1, -1, -1):
                    pw[i + 1] += of * pw[i] * dt((i + 1) / (k + 1))
                    pw[i] = z * pw[i] * dt((k - i) / (k + 1))
            for k in range(1, d + 1):
                z = Z[:, k - 1, None]; of = O[:, k - 1]
                zinv = np.divide(1.0, z, out=np.zeros_like(z), where=z != 0)
                nop = pw[d].copy(); tot = np.zeros_like(nop)
                for i in range(d - 1, -1, -1):
                    tmp = nop * dt((d + 1) / (i + 1))
                    nop = pw[i] - tmp * z * dt((d - i) / (d + 1))
                    tot += np.where(of > 0, tmp, pw[i] * zinv * dt((d + 1) / (d - i)))
                np.add.at(phi, feat[:, k - 1], tot * (of - z) * leaf[:, None])
    out[:, :nfeat] += phi.T
    out[:, nfeat] += base
    return out


def _mean_root(t):
    def m(n):
        if t["left"][n] == -1:
            return float(np.float32(t["cond"][n]))
        l, r = t["left"][n], t["right"][n]
        return (m(l) * t["cover"][l] + m(r) * t["cover"][r]) / t["cover"][n]
    return m(0)

def saabas64(trees, base, rows, missing, nfeat, ntree_limit=0):
    """Approximate mode's definition in float64 (1.6.0 CalculateContributionsApprox): along the row's path,
    mean(next) - mean(current) into the split feature's column, means from the covers; the bias is the sum of the root
    means + base.  Columns the matrix does not have are missing."""
    rows = _full_width(rows, nfeat)
    use = trees[:ntree_limit] if ntree_limit else trees
    ref = np.zeros((len(rows), nfeat + 1))
    for t in use:
        m = [0.0] * len(t["left"])

        def fill(n):
            if t["left"][n] == -1:
                m[n] = float(np.float32(t["cond"][n]))
            else:
                l, r = t["left"][n], t["right"][n]
                m[n] = (fill(l) * t["cover"][l] + fill(r) * t["cover"][r]) / t["cover"][n]
            return m[n]
        fill(0)
        for r, x in enumerate(rows):
            ref[r, nfeat] += m[0]
            n = 0
            while t["left"][n] != -1:
                f = t["feat"][n]
                miss = np.isnan(x[f]) or x[f] == missing
                nxt = (t["left"][n] if t["dl"][n] else t["right"][n]) if miss else \
                    (t["left"][n] if x[f] < np.float32(t["cond"][n]) else t["right"][n])
                ref[r, f] += m[nxt] - m[n]
                n = nxt
    ref[:, nfeat] += base
    return ref


def within(got, ref, rel=1e-5):
    """|got - ref| <= rel * (1 + sum_j |ref_j|) per row; returns the worst ratio to that bound."""
    bound = rel * (1.0 + np.sum(np.abs(ref), axis=1, keepdims=True))
    return float(np.max(np.abs(got.astype(np.float64) - ref) / bound)) if got.size else 0.0


# (ntree, nfeat, depth, p_leaf): stumps whose root is a leaf, chains, repeated features on deep paths, wider forests
CASES = [(1, 1, 0, 0.0), (3, 3, 1, 0.0), (4, 2, 6, 0.1), (6, 5, 5, 0.3), (5, 8, 8, 0.35), (8, 10, 6, 0.25),
         (2, 3, 12, 0.5)]
