"""References for the three pieces of the predict path that only decide which rows share a wave (test support):
the clustering keys and their `agree` words (csrc/kernels.hip cluster_keys_kernel), the rows' order the host reads from
them (csrc/kernels.hpp cluster_order) and the level search's verdict words (detect_period_kernel).  Whatever those
compute the margins stay bit-exact, so they are checked against what is written here.

The key (docs/30_cluster_and_level_search_tests.md).  Each of the key's `ntrees` trees contributes 1 + 2 * nsteps bits,
most significant first:
  * the root decision when the tree's phase is 1 (0 left, 1 right) - the walk moves to that child; phase 0: the bit is
    0 and the walk stays at the root;
  * then two bits per step, from the current node: a leaf gives 00 and the walk stays; otherwise b0 is the decision at
    the node, b1 the decision at that child (0 when the child is a leaf), and the walk moves to the grandchild or stays
    on the leaf; steps beyond the tree's trip count give 00.
A value is missing when it equals the marker, is NaN or its feature is >= ncol, and then goes where the node's default
says; otherwise the row goes left iff float32(x) < float32(cond).  Plain keys: the trees' parts concatenated, tree 0
highest.  z-order: the root bits on top (tree 0 highest), below them for each step and each tree within the step the
two bits.

`keys` walks the trees themselves (numpy over the rows); `keys_from_records` walks emit_super's records.  The two must
agree whatever the placement of the records: that is the check on the reference."""
import functools

import numpy as np

# (ntrees, nsteps, zorder) of the tests: one tree one step; 31 bits; the default; both orders of 3 and 4 trees
KEY_SHAPES = ((1, 1, 0), (1, 15, 0), (2, 7, 0), (2, 7, 1), (3, 4, 0), (3, 4, 1), (4, 3, 0), (4, 3, 1), (4, 1, 1))

FILLER_META = 0xE0          # csrc/flatten.cpp emit_super_tree: feature 0 three times, default left, group 0
_INF_BITS = 0x7F800000
_LESS = np.less             # (a test swaps in <= to show that its rows sit on thresholds the key decides at)


class _T:
    """A tree as arrays: tests.booster_shapes.Tree or an oracle.xgb_oracle.OracleTree."""

    def __init__(self, tree):
        if hasattr(tree, "cleft"):
            left, right, feat, cond, dl = tree.cleft, tree.cright, tree.feature, tree.value, tree.default_left
        else:
            left, right, feat, cond, dl = tree.left, tree.right, tree.feat, tree.cond, tree.dl
        self.left = np.asarray(left, dtype=np.int64)
        self.right = np.asarray(right, dtype=np.int64)
        self.feat = np.asarray(feat, dtype=np.int64)
        self.cond = np.asarray(cond, dtype=np.float64).astype(np.float32)
        self.dl = np.asarray(dl).astype(bool)


def _missing_mask(x, missing):
    m = np.isnan(x)
    return m if np.isnan(missing) else m | (x == np.float32(missing))


def _go_right(t, node, rows, ncol, missing):
    """The decision of every row at its node `node` (internal nodes; what it says of a leaf is discarded)."""
    f = t.feat[node]
    x = rows[np.arange(len(rows)), np.minimum(f, rows.shape[1] - 1)]
    miss = (f >= ncol) | _missing_mask(x, missing)
    with np.errstate(invalid="ignore"):
        left = np.where(miss, t.dl[node], _LESS(x, t.cond[node]))
    return ~left


def _compose(roots, steps, ntrees, nsteps, zorder):
    """roots[t]: (n,) 0/1; steps[t][s]: (n,) two bits -> keys (n,) uint32"""
    n = len(roots[0])
    key = np.zeros(n, dtype=np.uint64)
    if zorder:
        for t in range(ntrees):
            key |= roots[t].astype(np.uint64) << np.uint64(2 * nsteps * ntrees + (ntrees - 1 - t))
        for s in range(nsteps):
            for t in range(ntrees):
                key |= steps[t][s].astype(np.uint64) << np.uint64(2 * (nsteps * ntrees - 1 - (s * ntrees + t)))
    else:
        width = 1 + 2 * nsteps
        for t in range(ntrees):
            part = roots[t].astype(np.uint64) << np.uint64(2 * nsteps)
            for s in range(nsteps):
                part |= steps[t][s].astype(np.uint64) << np.uint64(2 * (nsteps - 1 - s))
            key |= part << np.uint64((ntrees - 1 - t) * width)
    assert ntrees * (1 + 2 * nsteps) <= 32 and int(key.max(initial=0)) < 1 << 32
    return key.astype(np.uint32)


def keys(trees, phases, rows, ncol, missing, ntrees, nsteps, zorder, stats=None):
    """The keys of `rows` ((n, >= ncol) float32; columns from ncol on are not there) from the trees themselves.
    phases: synth.super_heads_cpu's (phase, trip count) per tree.  stats: a dict that takes how many (row, step)
    pairs stood on a leaf, and how many reached one after b0 only."""
    rows = np.asarray(rows, dtype=np.float32)[:, :max(ncol, 1)]
    n = len(rows)
    roots, steps = [], []
    for ti in range(ntrees):
        t = _T(trees[ti])
        phase, trips = int(phases[ti][0]), int(phases[ti][1])
        node = np.zeros(n, dtype=np.int64)
        root = np.zeros(n, dtype=np.uint32)
        if phase == 1:
            assert t.left[0] != -1
            r = _go_right(t, node, rows, ncol, missing)
            root = r.astype(np.uint32)
            node = np.where(r, t.right[node], t.left[node])
        mine = []
        for s in range(nsteps):
            if s >= trips:
                mine.append(np.zeros(n, dtype=np.uint32))
                continue
            leaf = t.left[node] == -1
            b0 = ~leaf & _go_right(t, node, rows, ncol, missing)
            child = np.where(leaf, node, np.where(b0, t.right[node], t.left[node]))
            child_leaf = t.left[child] == -1
            b1 = ~child_leaf & _go_right(t, child, rows, ncol, missing)
            node = np.where(child_leaf, child, np.where(b1, t.right[child], t.left[child]))
            if stats is not None:
                stats["leaf_after_b0"] = stats.get("leaf_after_b0", 0) + int((~leaf & child_leaf).sum())
                stats["on_a_leaf"] = stats.get("on_a_leaf", 0) + int(leaf.sum())
            mine.append(b0.astype(np.uint32) * 2 + b1.astype(np.uint32))
        roots.append(root)
        steps.append(mine)
    return _compose(roots, steps, ntrees, nsteps, zorder)


def keys_from_records(nodes, heads, rows, ncol, missing, ntrees, nsteps, zorder, fillers="stay"):
    """The same keys from emit_super's arrays (synth.super_records_cpu: nodes [records][4] = thr0, thrL, thrR bits and
    meta, heads [trees][4] = base, root_meta, root_thr bits, trip count), a step at a time as the comment above the
    kernel describes: two decisions per record, next = base + 4 * group + 2 * b0 + b1, a record whose own node is a
    leaf (code 31) gives 00 and leads to group 0, fillers give 00 and lead to fillers.
    fillers="walk": a filler is read like any record (feature 0 against +inf) - what the kernel did until this was
    written; it differs exactly where a row holds +inf, not as the missing marker, in feature 0."""
    rows = np.asarray(rows, dtype=np.float32)[:, :max(ncol, 1)]
    n = len(rows)
    nodes = np.asarray(nodes, dtype=np.uint32)
    thr = nodes[:, :3].copy().view(np.float32)
    meta = nodes[:, 3].astype(np.int64)
    is_filler = (meta == FILLER_META) & np.all(nodes[:, :3] == _INF_BITS, axis=1)
    at = np.arange(n)

    def decide(f, cond, default_left):
        x = rows[at, np.minimum(f, rows.shape[1] - 1)]
        miss = (f >= ncol) | _missing_mask(x, missing)
        with np.errstate(invalid="ignore"):
            return ~np.where(miss, default_left, _LESS(x, cond))

    roots, steps = [], []
    for ti in range(ntrees):
        base, root_meta, _, trips = (int(v) for v in heads[ti])
        root_thr = heads[ti:ti + 1, 2].copy().view(np.float32)[0]
        rel = np.full(n, 4, dtype=np.int64)
        root = np.zeros(n, dtype=np.uint32)
        if root_meta & 0x100:
            r = decide(np.full(n, root_meta & 31, dtype=np.int64), root_thr, np.full(n, bool(root_meta & 32)))
            root = r.astype(np.uint32)
            rel = rel + r
        mine = []
        for s in range(nsteps):
            if s >= trips:
                mine.append(np.zeros(n, dtype=np.uint32))
                continue
            rec = base + rel
            w = meta[rec]
            f0 = (w >> 8) & 31
            on_leaf = f0 == 31
            if fillers == "stay":
                on_leaf = on_leaf | is_filler[rec]
            b0 = ~on_leaf & decide(f0, thr[rec, 0], (w & 32) != 0)
            f1 = np.where(b0, (w >> 13) & 31, w & 31)
            b1 = ~on_leaf & (f1 != 31) & decide(f1, np.where(b0, thr[rec, 2], thr[rec, 1]),
                                                np.where(b0, (w & 128) != 0, (w & 64) != 0))
            rel = (w >> 18) * 4 + b0 * 2 + b1           # (a leaf's record and a filler name group 0)
            mine.append(b0.astype(np.uint32) * 2 + b1.astype(np.uint32))
        roots.append(root)
        steps.append(mine)
    return _compose(roots, steps, ntrees, nsteps, zorder)


def leads(key, ntrees, nsteps, zorder):
    """The root bit and the two bits of step 0 of tree 0, out of a key: what `agree` is counted on."""
    key = np.asarray(key, dtype=np.uint64)
    if zorder:
        root = (key >> np.uint64(2 * nsteps * ntrees + ntrees - 1)) & np.uint64(1)
        step0 = (key >> np.uint64(2 * (nsteps * ntrees - 1))) & np.uint64(3)
        return ((root << np.uint64(2)) | step0).astype(np.uint32)
    width = 1 + 2 * nsteps
    return ((key >> np.uint64((ntrees - 1) * width + 2 * (nsteps - 1))) & np.uint64(7)).astype(np.uint32)


def agree(lead, nrow):
    """The nine words: [0] rows r with r % 64 != 0 whose lead equals row r - 1's, [1..8] the histogram of lead & 7."""
    lead = np.asarray(lead, dtype=np.uint32)
    assert len(lead) == nrow
    same = lead[1:] == lead[:-1]
    same &= (np.arange(1, nrow) % 64) != 0
    out = np.zeros(9, dtype=np.uint32)
    out[0] = int(same.sum())
    out[1:] = np.bincount(lead & 7, minlength=8)
    assert int(out[1:].sum()) == nrow
    return out


def order(words, nrow):
    """-> (order, observed, by_chance): the header's formula in Python floats."""
    n = float(nrow)
    observed = float(words[0]) / n
    by_chance = 0.0
    for v in range(1, 9):
        by_chance += (float(words[v]) / n) * (float(words[v]) / n)
    return ((observed - by_chance) / (1.0 - by_chance) if by_chance < 0.999 else 0.0), observed, by_chance


def period_verdict(data, cols, kmax):
    """verdict[c][x] for the periods nrow / (kmax - x): 2 where kmax - x does not divide nrow or the column is not
    there, 0 where the column repeats bit for bit with that period, 1 where the first pair, the last pair or at least
    half of all pairs differ.  Anything in between is not part of the contract (the kernel samples pairs) and raises."""
    data = np.ascontiguousarray(data, dtype=np.float32)
    nrow, ncol = data.shape
    bits = data.view(np.uint32)
    out = np.zeros((len(cols), kmax - 1), dtype=np.uint32)
    for c, col in enumerate(cols):
        for x in range(kmax - 1):
            k = kmax - x
            if nrow % k or col >= ncol:
                out[c, x] = 2
                continue
            p = nrow // k
            diff = bits[:-p, col] != bits[p:, col]
            if not diff.any():
                out[c, x] = 0
            elif diff[0] or diff[-1] or 2 * int(diff.sum()) >= len(diff):
                out[c, x] = 1
            else:
                raise AssertionError(f"column {col}, k = {k}: {int(diff.sum())} of {len(diff)} pairs differ, neither "
                                     "end among them: the contract says nothing about this matrix")
    return out


# ---- the boosters and rows of the tests, made once ----

def is_root_leaf(tree):
    return int(_T(tree).left[0]) == -1


def _shape_tree(oracle_tree):
    """An OracleTree as a tests.booster_shapes.Tree (what tie_rows leads its rows down)."""
    from tests import booster_shapes as S
    t = S.Tree()
    t.left, t.right = [int(v) for v in oracle_tree.cleft], [int(v) for v in oracle_tree.cright]
    t.feat, t.cond = [int(v) for v in oracle_tree.feature], [float(v) for v in oracle_tree.value]
    t.dl = [int(v) for v in oracle_tree.default_left]
    t.hess = [1.0] * len(t.left)
    return t


@functools.lru_cache(maxsize=None)
def booster(name):
    """-> (image, [Tree], heads): S.make_booster(1000 + n, n) for a number, "synth": the benchmark booster's shape
    (20 trees of depth <= 18, nearly full, every tree of phase 1).  heads: synth.super_heads_cpu's (phase, trips)."""
    from oracle import xgb_oracle as O
    from quickchem_amd import synth
    from tests import booster_shapes as S
    if name == "synth":
        image = synth.make_model(num_trees=20, max_depth=18, sample_log2=16, min_leaf=2).image
        trees = [_shape_tree(t) for t in O.load_model(bytes(image)).trees]
    else:
        image, trees = S.make_booster(1000 + name, name)
    heads = synth.super_heads_cpu(image)
    assert heads is not None and len(heads) == len(trees)
    return image, trees, heads


def _top(tree, depth):
    """The tree cut below `depth` levels of splits (a booster_shapes.Tree): what a short key sees of it."""
    from tests import booster_shapes as S
    t = S.Tree()
    todo = [(0, t.node(), 0)]
    while todo:
        src, dst, d = todo.pop()
        t.cond[dst] = tree.cond[src]
        if tree.left[src] == -1 or d >= depth:
            continue
        t.feat[dst], t.dl[dst] = tree.feat[src], tree.dl[src]
        l, r = t.split(dst)
        todo += [(tree.left[src], l, d + 1), (tree.right[src], r, d + 1)]
    return t


@functools.lru_cache(maxsize=None)
def _rows(name, missing_bits):
    from tests import booster_shapes as S
    missing = float(np.array([missing_bits], dtype=np.uint32).view(np.float32)[0])
    seed = 77 if name == "synth" else name
    key_trees = booster(name)[1][:4]
    rows = S.rows_for(seed, key_trees, 3000, missing)
    tops = [_top(t, 3) for t in key_trees]
    if any(t.left[0] != -1 for t in tops):
        rows[2250:] = S.tie_rows(np.random.default_rng(seed + 1), tops, 750)
    rows.setflags(write=False)
    return rows


WIRING_ROWS = (1 << 18) + 1000      # csrc/capi.cpp cluster_rows: from 2^18 rows on the order is judged


@functools.lru_cache(maxsize=None)
def wiring_batches():
    """[(booster name, rows)] of the wiring test: rows in grid order from a ragged C48 shard (no level size divides
    them) under the benchmark-shaped booster; the same rows shuffled; the shuffled rows under the booster whose first
    tree is a root leaf."""
    from quickchem_amd import synth
    grid = synth.GRIDS["C48"]
    assert WIRING_ROWS % (grid[0] * grid[1]) != 0 and is_root_leaf(booster(135)[1][0])
    ordered = synth.rows_cpu(grid, 123_456, WIRING_ROWS)
    shuffled = np.ascontiguousarray(ordered[np.random.default_rng(5).permutation(WIRING_ROWS)])
    return (("synth", ordered), ("synth", shuffled), (135, shuffled))


def wiring_child(out_path):
    """What the child process of the wiring test runs: the three batches through OHXBoosterPredictDevice with
    ohx_cluster left on auto, each on a matrix of its own; margins_1 .. margins_3 into an .npz.  The verdicts go to
    stderr (OHX_DEBUG)."""
    import torch
    from quickchem_amd import capi, synth
    margins = {}
    for i, (name, batch) in enumerate(wiring_batches(), 1):
        b = capi.Booster(model_buffer=booster(name)[0])
        t = torch.from_numpy(batch).cuda()
        d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=batch.shape[0], ncol=batch.shape[1], missing=synth.XX_MISS)
        out = torch.zeros(batch.shape[0], dtype=torch.float32, device="cuda")
        b.predict_device(d, out.data_ptr())
        torch.cuda.synchronize()
        b.check()
        assert d.grid() == (0, 0, 0, False)
        margins["margins_%d" % i] = out.cpu().numpy()
        d.free()
        b.free()
    np.savez(out_path, **margins)


def rows(name, missing):
    """3000 rows for booster(name): random rows (NaN, -999.0, special values, both infinities where the marker is one)
    and, as the second half, tie rows that sit on thresholds of the trees a key can be made of (its first four) - the
    last 750 of them on the three levels of splits that even the shortest key decides at.  Read-only, shared."""
    return _rows(name, int(np.array([missing], dtype=np.float32).view(np.uint32)[0]))
