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


def with_covers(rng, left, right):
    """Leaves get a random integer cover, a split the sum of its children's: then mean(root) == v({})."""
    n = len(left)
    cover = [0.0] * n

    def fill(i):
        if left[i] == -1:
            cover[i] = float(rng.integers(1, 50))
        else:
            cover[i] = fill(left[i]) + fill(right[i])
        return cover[i]
    fill(0)
    return cover


def random_booster(rng, ntree, nfeat, max_depth, p_leaf, base_score=None):
    """(json bytes, trees, base) - trees as dicts of python lists, for the brute force."""
    return booster_from_trees(rng, [random_tree(rng, nfeat, max_depth, p_leaf) for _ in range(ntree)], nfeat,
                              base_score)


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


def booster_from_trees(rng, shapes, nfeat, base_score=None):
    ntree = len(shapes)
    trees, docs = [], []
    for t, (left, right, feat, cond, dl) in enumerate(shapes):
        cover = with_covers(rng, left, right)
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
            if k is None: path.append({"f":f,"lo":-np.inf,"hi":np.inf,"m":True,"z":1.0}); k=len(path)-1
            e=path[k]
            if side==0: e["hi"]=min(e["hi"],c)
            else: e["lo"]=max(e["lo"],c)
            e["m"]=e["m"] and miss; e["z"]*=z
            walk(ch,path)
            path[:]=old
    walk(0,[])
    return out

def treeshap64(trees, base, rows, missing, nfeat):
    """Path-dependent TreeSHAP in float64, path by path as the kernels evaluate it (one element per distinct feature,
    intervals, merged zero fractions) - exact to float64 rounding, so a reference where the brute force cannot go
    (more than 10 features); checked against the brute force in test_contribs_cpu.py."""
    dt = np.float64
    n=len(rows); out=np.zeros((n,nfeat+1),dt)
    miss_all = np.isnan(rows) | (rows==missing)
    for t in trees:
        tc=np.zeros((n,nfeat),dt)
        for path, v in _paths_of(t):
            d=len(path)
            o=[]
            for e in path:
                x=rows[:,e["f"]]
                o.append(np.where(miss_all[:,e["f"]], e["m"], (x>=e["lo"])&(x<e["hi"])).astype(dt))
            pw=np.zeros((d+1,n),dt); pw[0]=1
            for k in range(1,d+1):
                z=dt(path[k-1]["z"]); of=o[k-1]
                for i in range(k-1,-1,-1):
                    pw[i+1]+=of*pw[i]*dt((i+1)/(k+1))
                    pw[i]=z*pw[i]*dt((k-i)/(k+1))
            for k in range(1,d+1):
                z=dt(path[k-1]["z"]); of=o[k-1]
                nop=pw[d].copy(); tot=np.zeros(n,dt)
                for i in range(d-1,-1,-1):
                    tmp=nop*dt((d+1)/(i+1))
                    nop=pw[i]-tmp*z*dt((d-i)/(d+1))
                    tot+=np.where(of>0,tmp,pw[i]/z*dt((d+1)/(d-i)))
                tc[:,path[k-1]["f"]]+=tot*(of-z)*dt(np.float32(v))
        out[:, :nfeat] += tc
        out[:, nfeat] += _mean_root(t)
    out[:, nfeat] += base
    return out


def _mean_root(t):
    def m(n):
        if t["left"][n] == -1:
            return float(np.float32(t["cond"][n]))
        l, r = t["left"][n], t["right"][n]
        return (m(l) * t["cover"][l] + m(r) * t["cover"][r]) / t["cover"][n]
    return m(0)

def within(got, ref, rel=1e-5):
    """|got - ref| <= rel * (1 + sum_j |ref_j|) per row; returns the worst ratio to that bound."""
    bound = rel * (1.0 + np.sum(np.abs(ref), axis=1, keepdims=True))
    return float(np.max(np.abs(got.astype(np.float64) - ref) / bound)) if got.size else 0.0


# (ntree, nfeat, depth, p_leaf): stumps whose root is a leaf, chains, repeated features on deep paths, wider forests
CASES = [(1, 1, 0, 0.0), (3, 3, 1, 0.0), (4, 2, 6, 0.1), (6, 5, 5, 0.3), (5, 8, 8, 0.35), (8, 10, 6, 0.25),
         (2, 3, 12, 0.5)]
