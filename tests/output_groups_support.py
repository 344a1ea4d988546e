"""Boosters with several output groups (multi-class, multi-target) for the output-group tests, and their decomposition
into single-group boosters: group g's trees, in file order, with the same base_score.  The oracle and the single-group
paths are pinned elsewhere; a multi-group booster is checked against its parts."""
import json

import numpy as np

from tests import booster_shapes as S

PATTERNS = ("round_robin", "blocked", "irregular", "one_empty")


def tree_info_for(pattern, ntree, G, seed=0):
    """Output group of each tree.  one_empty: group 1 (of G) has no tree."""
    rng = np.random.default_rng(seed)
    if pattern == "round_robin":
        return [t % G for t in range(ntree)]
    if pattern == "blocked":
        return [t * G // ntree for t in range(ntree)]
    if pattern == "irregular":
        info = [int(g) for g in rng.integers(0, G, ntree)]
        info[:G] = list(range(G))[:ntree]          # every group holds a tree ...
        rng.shuffle(info)                         # ... somewhere
        return info
    if pattern == "one_empty":
        others = [g for g in range(G) if g != 1]
        return [others[t % len(others)] for t in range(ntree)]
    raise ValueError(pattern)


def multi_json(image, tree_info, G, objective="multi:softprob", multi_target=False):
    """A booster_json image turned into one of G output groups: tree_info, num_class (or num_target), objective."""
    doc = json.loads(bytes(image))
    learner = doc["learner"]
    learner["gradient_booster"]["model"]["tree_info"] = [int(g) for g in tree_info]
    lmp = learner["learner_model_param"]
    if multi_target:
        lmp["num_class"], lmp["num_target"] = "0", str(G)
    else:
        lmp["num_class"], lmp["num_target"] = str(G), "1"
    learner["objective"] = {"name": objective}
    if objective.startswith("multi:"):
        learner["objective"]["softmax_multiclass_param"] = {"num_class": str(G)}
    return json.dumps(doc).encode()


def sub_json(image, tree_info, g):
    """The single-group booster of group g's trees in file order (reg:squarederror, the same base_score), or None for a
    group without trees."""
    doc = json.loads(bytes(image))
    model = doc["learner"]["gradient_booster"]["model"]
    keep = [t for t, gi in zip(model["trees"], tree_info) if gi == g]
    if not keep:
        return None
    for i, t in enumerate(keep):
        t["id"] = i
    model["trees"] = keep
    model["tree_info"] = [0] * len(keep)
    model["gbtree_model_param"]["num_trees"] = str(len(keep))
    lmp = doc["learner"]["learner_model_param"]
    lmp["num_class"], lmp["num_target"] = "0", "1"
    doc["learner"]["objective"] = {"name": "reg:squarederror", "reg_loss_param": {"scale_pos_weight": "1"}}
    return json.dumps(doc).encode()


def base_margin(image):
    return np.float32(float(json.loads(bytes(image))["learner"]["learner_model_param"]["base_score"]))


def group_counts(tree_info, G, ntree_limit):
    """Trees of each group among the file trees a call with this ntree_limit uses: [0, min(T, k * G))."""
    T = len(tree_info)
    L = T if ntree_limit == 0 or ntree_limit * G > T else ntree_limit * G
    return [sum(1 for t in range(L) if tree_info[t] == g) for g in range(G)], L


def make_multi(seed, ntree, G, pattern, objective="multi:softprob", multi_target=False, contribs=False, rows=None):
    """-> (multi-group image, [Tree], tree_info)."""
    if contribs:
        image, trees = S.contribs_booster(seed, ntree)
    else:
        image, trees = S.make_booster(seed, ntree, rows=rows)
    info = tree_info_for(pattern, ntree, G, seed)
    return multi_json(image, info, G, objective, multi_target), trees, info


# ---- margins that are exact by construction, for the transforms (groups.hip group_finish_kernel) ----

# differences within a row: ties, one float32 step, and the ranges where expf leaves the normal floats (about 87.3),
# the denormals (about 103.97) and reaches 0
DIFFERENCES = ("0", "ulp", 10.0, 87.3, 88.8, 103.9, 104.1, 200.0, 1e30, "signed_zero")


def engineered_leaves(G, diff, top=0):
    """-> float32 [G]: the leaf value of every group's root-leaf tree.  Group `top` holds the largest one, a, the others
    a - diff in turn with a itself (so the maximum is tied in several groups where G > 2)."""
    if diff == "signed_zero":
        v = np.where(np.arange(G) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        if top:
            v = -v
        return v
    a = np.float32(1e30) if diff == 1e30 else np.float32(1.0)
    if diff == "0":
        low = a
    elif diff == "ulp":
        low = np.nextafter(a, np.float32(0))
    else:
        low = np.float32(a - np.float32(diff))
    v = np.where((np.arange(G) - top) % 2 == 0, a, low).astype(np.float32)
    if G > 2:
        v[(top + 2) % G] = np.float32(low)        # ... and not every second group ties with the first
        v[top] = a
    return v


def engineered_booster(G, diff, top=0, objective="multi:softprob", base=-0.0, multi_target=False):
    """-> (image, leaves [G], step): G root leaves (group g's is leaves[g]) and, in the LAST group, a stump on feature 0
    at 0.0 whose left leaf is -0.0 (x + -0.0 is x for every x, -0.0 included) and whose right leaf is `step` = the largest difference between the leaves: rows with
    x0 >= 0 lift the last group to a tie with the largest margin, or past it by that difference.  base_score is -0.0, which keeps a leaf of -0.0 a
    margin of -0.0 (+0.0 + -0.0 would be +0.0)."""
    leaves = engineered_leaves(G, diff, top)
    step = np.float32(leaves.max() - leaves.min())
    trees = []
    for g in range(G):
        t = S.Tree()
        t.node()
        t.cond[0] = float(leaves[g])
        trees.append(t)
    t = S.Tree()
    root = t.node()
    l, r = t.split(root)
    t.feat[root], t.cond[root], t.dl[root] = 0, 0.0, 1
    t.cond[l], t.cond[r] = -0.0, float(step)
    trees.append(t)
    image = S.booster_json(trees, np.float32(base))
    doc = json.loads(image)
    doc["learner"]["learner_model_param"]["base_score"] = "-0" if (base == 0 and np.signbit(base)) else "%.9g" % base
    image = json.dumps(doc).encode()
    info = list(range(G)) + [G - 1]
    return multi_json(image, info, G, objective, multi_target), leaves, step


def engineered_margins(leaves, step, rows, base=-0.0):
    """[nrow][G] float32: base + leaf, and in the last group + the stump's leaf, added in float32 in file order."""
    G = len(leaves)
    m = np.empty((len(rows), G), dtype=np.float32)
    for g in range(G):
        m[:, g] = np.float32(base) + np.float32(leaves[g])
    lift = np.where(rows[:, 0] < np.float32(0.0), np.float32(-0.0), np.float32(step)).astype(np.float32)
    m[:, G - 1] = (m[:, G - 1] + lift).astype(np.float32)
    return m


def engineered_rows(n=130):
    """Rows whose feature 0 lies on both sides of the stump's 0.0, -0.0 and 0.0 themselves included (no missing)."""
    rng = np.random.default_rng(1)
    rows = rng.normal(0, 1, (n, S.NFEAT)).astype(np.float32)
    rows[:4, 0] = np.array([-0.0, 0.0, -1e-45, 1e-45], dtype=np.float32)
    return rows


def softprob_reference(m):
    """1.6.0's common::Softmax on float32 margins, in float64 from the FLOAT32 difference m_g - max (the subtraction is
    made in float there, so its rounding belongs to the operation): the float64 exp of it, the float64 sum in group
    order, the sum rounded to float32 (the divisor is a float), the quotient.  -> float64 [nrow][G]."""
    m = np.asarray(m, dtype=np.float32)
    d = (m - m.max(axis=1, keepdims=True)).astype(np.float32)
    e = np.exp(d.astype(np.float64))
    s = np.zeros(len(m), dtype=np.float64)
    for g in range(m.shape[1]):
        s += e[:, g]
    return e / s.astype(np.float32).astype(np.float64)[:, None]


def softprob_float32(m):
    """The same formula as a float32 program would evaluate it: expf, a double sum, a float divisor, a float quotient."""
    m = np.asarray(m, dtype=np.float32)
    e = np.exp((m - m.max(axis=1, keepdims=True)).astype(np.float32)).astype(np.float32)
    s = np.zeros(len(m), dtype=np.float64)
    for g in range(m.shape[1]):
        s += e[:, g].astype(np.float64)
    return (e / s.astype(np.float32)[:, None]).astype(np.float32)


def softprob_excess_ulp(prob, ref):
    """|prob - ref| in float32 ulp of ref (np.spacing: 2**-149 in the denormal range and at 0)."""
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(prob, dtype=np.float64) - ref) / ulp
