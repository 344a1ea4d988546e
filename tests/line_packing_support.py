"""Boosters for the tests of the super-node group placement ("ohx_super_pack", csrc/flatten.hpp kSuperPack*), and the
checks of what flatten.hpp promises read back from emit_super's own arrays (test support).

The shapes are those at which a wrong group number, a misplaced filler or a base off by one group shows:
  stump         no group below the start
  left / right  a depth-10 chain that always goes on to the left (right): only one child is ever internal, every deep group
                is a single
  complete      a complete depth-10 tree: every deep group has all four records, every pair is a sibling pair
  parity        three trees whose group counts are odd, odd and even: the second and the third would start on an odd group
  phases        a phase-0 and a phase-1 tree side by side
  cap           one tree of 15 724 groups breadth first that passes kSuperMaxGroups (16 384) only with the groups the
                families skip: it keeps its super-nodes and, for that variant, the old numbers
  random        8 random lopsided trees of depth 12 (the GPU tests)
Thresholds are values of the rows the booster is made for, or one float32 step either side (booster_shapes.neighbour)."""
import functools

import numpy as np

from quickchem_amd import synth
from tests import booster_shapes as S
from tests.test_random_forests import random_tree

PACKS = synth.SUPER_PACKS
MAX_GROUPS = 1 << 14
FILLER = np.array([0x7F800000, 0x7F800000, 0x7F800000, 0xE0], dtype=np.uint32)   # +inf three times, default left, group 0


def _complete(t, n, depth):
    """a complete subtree of `depth` levels below node n -> its leaves"""
    frontier = [n]
    for _ in range(depth):
        frontier = [c for m in frontier for c in t.split(m)]
    return frontier


def _chain(depth, go_left):
    t = S.Tree()
    n = t.node()
    for _ in range(depth):
        l, r = t.split(n)
        n = l if go_left else r
    return t


def _complete_tree(depth):
    t = S.Tree()
    _complete(t, t.node(), depth)
    return t


def _cap_tree():
    """Complete to depth 16 (every leaf at an even depth: phase 1, records on the odd depths, 10 924 groups), then 1 600
    groups of the last level's records - the records of one group follow each other among the depth-15 nodes - get a
    child group under three of their four records: 15 724 groups breadth first, a third more of those 4 800 with a
    256-byte stretch each."""
    t = S.Tree()
    leaves = _complete(t, t.node(), 16)                # in breadth-first order: four consecutive depth-15 nodes' children
    for g in range(1600):
        for rec in range(3):
            # the record on depth-15 node number 4 g + rec: its left child (a depth-16 leaf) becomes internal
            t.split(leaves[2 * (4 * g + rec)])
    return t


def _random_tree(rng, depth):
    left, right, _, _, _ = random_tree(rng, S.NFEAT, depth, 0.3)
    t = S.Tree()
    t.left, t.right = list(left), list(right)
    n = len(left)
    t.feat, t.cond, t.dl, t.hess = [0] * n, [0.0] * n, [0] * n, [1.0] * n
    return t


def _fill(rng, t, pool, phase):
    """features, thresholds from the pool (per feature, sorted unique finite values), default directions, leaf values"""
    n = len(t.left)
    feat = rng.integers(0, S.NFEAT, n)
    cond = np.empty(n, dtype=np.float32)
    for f in range(S.NFEAT):
        m = feat == f
        cond[m] = pool[f][rng.integers(0, len(pool[f]), int(m.sum()))]
    step = rng.integers(0, 3, n)
    up, down = np.nextafter(cond, np.float32(np.inf)), np.nextafter(cond, np.float32(-np.inf))
    cond = np.where((step == 1) & np.isfinite(down), down, np.where((step == 2) & np.isfinite(up), up, cond))
    leaf = np.array(t.left) == -1
    cond[leaf] = rng.normal(0, 0.1, int(leaf.sum())).astype(np.float32)
    feat[leaf] = 0
    t.feat, t.cond = [int(x) for x in feat], [float(x) for x in cond]
    t.dl = [int(x) for x in np.where(leaf, 0, rng.integers(0, 2, n))]
    S._force_phase(rng, t, phase)
    return t


def _groups(js):
    """groups of a one-tree booster, numbered breadth first"""
    rec = synth.super_records_cpu(js, 0)
    return (len(rec["nodes"]) - 48) // 4


def make_forests(rows, seed=5, which=None):
    """-> {name: (JSON image, [Tree])}; thresholds from `rows`"""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, dtype=np.float32)
    pool = []
    for c in rows.T:
        v = np.unique(c[np.isfinite(c)]).astype(np.float32)
        pool.append(v if len(v) else np.zeros(1, dtype=np.float32))

    def booster(trees):
        return S.booster_json(trees, np.float32(rng.normal(0, 1))), trees
    out = {}
    out["stump"] = booster([_fill(rng, _chain(1, True), pool, 0)])
    out["left"] = booster([_fill(rng, _chain(10, True), pool, 0)])
    out["right"] = booster([_fill(rng, _chain(10, False), pool, 1)])
    out["complete"] = booster([_fill(rng, _complete_tree(10), pool, 0)])
    # group counts odd, odd, even: lopsided random trees, taken as their counts come
    need, got = [1, 1, 0], []
    for _ in range(200):
        t = _fill(rng, _random_tree(rng, 11), pool, int(rng.integers(0, 2)))
        if len(got) < 3 and len(t.left) > 300 and _groups(S.booster_json([t], 0.0)) % 2 == need[len(got)]:
            got.append(t)
    assert len(got) == 3
    out["parity"] = booster(got)
    out["phases"] = booster([_fill(rng, _complete_tree(9), pool, 0), _fill(rng, _complete_tree(10), pool, 1)])
    if which is None or "cap" in which:
        out["cap"] = booster([_fill(rng, _cap_tree(), pool, 1)])
    if which is None or "random" in which:
        out["random"] = booster([_fill(rng, _random_tree(rng, 12), pool, i & 1) for i in range(8)])
    return out if which is None else {k: v for k, v in out.items() if k in which}


# ---- what flatten.hpp promises, read from emit_super's arrays ----

def check_layout(rec, pack, may_fall_back=False):
    """rec: synth.super_records_cpu.  Group 0 four fillers; the start in group 1; a slot below a leaf a filler (which
    leads to group 0); no group named twice or outside its tree; the records of levels 0 - 3 within the tree's first
    176; tree bases on a line for pack >= 1; below level 3 the child groups of sibling records share a line for
    pack >= 2 (a tree that kept the old numbers excepted).  -> (trees numbered by line, sibling pairs checked)"""
    nodes, heads, packed = rec["nodes"], rec["heads"], rec["packed"]
    assert len(nodes) >= 48 and (nodes[-48:] == FILLER).all(), "the padding behind the last tree"
    meta = nodes[:, 3]
    filler = (nodes == FILLER).all(axis=1)
    f0, fl, fr, grp = (meta >> 8) & 31, meta & 31, (meta >> 13) & 31, meta >> 18
    pairs = 0
    for t in range(len(heads)):
        base = int(heads[t, 0])
        end = int(heads[t + 1, 0]) if t + 1 < len(heads) else len(nodes) - 48
        assert base % (8 if pack >= 1 else 4) == 0, (t, base)
        ngroups = (end - base) // 4
        assert ngroups >= 2 and ngroups <= MAX_GROUPS + 1                 # (+ 1: the filler group in front of the next tree)
        assert filler[base:base + 4].all(), "group 0"
        phase = (int(heads[t, 1]) >> 8) & 1
        assert not filler[base + 4] and (not filler[base + 5]) == (phase == 1) and filler[base + 6:base + 8].all(), "group 1"
        if not may_fall_back:
            assert packed[t] == (1 if pack >= 2 else 0)
        seen = set()
        level = {4: 0, 5: 0} if phase else {4: 0}
        frontier = sorted(level)
        while frontier:
            nxt = []
            for rel in frontier:
                r = base + rel
                assert not filler[r]
                g = int(grp[r])
                if level[rel] <= 3:
                    assert rel < 176, (t, rel, level[rel])
                if f0[r] == 31:
                    assert g == 0 and fl[r] == 31 and fr[r] == 31, "a leaf on top"
                    continue
                if g == 0:
                    assert fl[r] == 31 and fr[r] == 31, "no child group: both children are leaves"
                    continue
                assert 2 <= g < ngroups and g not in seen, (t, rel, g)
                seen.add(g)
                for side, code in ((0, fl[r]), (2, fr[r])):
                    for s in (side, side + 1):
                        c = 4 * g + s
                        if code == 31:
                            assert filler[base + c], "a slot below a leaf"
                        else:
                            assert not filler[base + c]
                            level[c] = level[rel] + 1
                            nxt.append(c)
            frontier = nxt
        assert int(heads[t, 3]) == max(level.values()) + 1, "steps"
        # every other record of the tree is a filler
        used = np.zeros(end - base, dtype=bool)
        used[list(level)] = True
        assert filler[base:end][~used].all()
        if pack >= 2 and packed[t]:
            for rel, lv in level.items():
                if lv >= 3 and rel % 2 == 0 and rel + 1 in level:
                    a, b = int(grp[base + rel]), int(grp[base + rel + 1])
                    if a and b:
                        assert a ^ b == 1, (t, rel, a, b)
                        pairs += 1
    return int(packed.sum()), pairs
