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
