"""The adversarial boosters of tests/booster_shapes.py on the host: they reach the edge classes they are made for (read
back through emit_super's own tree heads), and the super-node layout walked the kernels' way agrees with both oracles
on them, bit for bit, for every missing marker."""
import numpy as np
import pytest

from oracle import xgb_oracle as O
from quickchem_amd import synth
from tests import booster_shapes as S
from tests import helpers

COUNTS = (1, 2, 3, 5, 10, 135)
MISSING = (-999.0, float("nan"), float("inf"), float("-inf"))


def test_the_adversarial_boosters_reach_the_kernels_edges():
    every = []
    for ntree in COUNTS:
        js, trees = S.make_booster(1000 + ntree, ntree)
        heads = synth.super_heads_cpu(js)
        assert heads is not None and len(heads) == ntree
        phase, steps = heads[:, 0].astype(int), heads[:, 1].astype(int)
        for t, tree in enumerate(trees):
            if tree.left[0] == -1:                              # a root leaf: phase 0, one step
                assert (phase[t], steps[t]) == (0, 1)
        if ntree % 4 and ntree > 1:
            # the last group of 1 - 3 trees (its other chains repeat the last tree) holds trees of unequal depth
            last = steps[ntree - ntree % 4:]
            assert len(set(last)) > 1 or ntree % 4 == 1, (ntree, last)
        every.append((ntree, trees, phase, steps))
    _, trees, phase, steps = every[-1]
    # the big booster alone reaches every class
    assert any(t.left[0] == -1 for t in trees), "root leaves"
    assert np.any((phase == 0) & (steps >= 5)) and np.any((phase == 1) & (steps >= 5)), "both phases with >= 5 steps"
    assert np.any(steps == 4) and np.any(steps == 5), "exactly 4 and exactly 5 steps (the last LDS step, the first gathered one)"
    assert steps.max() >= 12 and steps.max() <= 16, steps.max()
    groups = [steps[g:g + 4] for g in range(0, len(steps), 4)]
    assert any(g.min() < 4 < g.max() for g in groups), "a group whose steps straddle 4"
    # chain 0 shallower than the group's deepest, which walks past the LDS steps (the trip count is the group's max)
    assert any(max(4, g[0]) < g.max() for g in groups)
    assert any(len(set(np.sign(g - 4.5))) > 1 and len(set(phase[4 * q:4 * q + 4])) > 1 for q, g in enumerate(groups)), \
        "a group that mixes phases and both sides of 4 steps"
    assert len(trees) > 128
    for ntree in (3, 10):                        # last group of 3 / 2 trees of unequal depth, one beyond 4 steps
        st = [e for e in every if e[0] == ntree][0][3]
        assert st[-(ntree % 4):].max() > 4 and len(set(st[-(ntree % 4):])) > 1


@pytest.mark.parametrize("ntree", COUNTS)
@pytest.mark.parametrize("missing", MISSING)
def test_super_walk_matches_both_oracles_on_adversarial_boosters(ntree, missing):
    js, trees = S.make_booster(1000 + ntree, ntree)
    binary = synth.convert_model(js, "binary")
    rows = S.rows_for(ntree, trees, 3000, missing)
    tie = rows[1500:]
    assert np.isfinite(tie).all()
    if np.isinf(missing):
        assert np.isposinf(rows).any() and np.isneginf(rows).any()
    want = helpers.oracle_predict(binary, rows, missing)
    assert np.array_equal(helpers.bits(O.predict(O.load_model(js), rows, missing=missing)), helpers.bits(want))
    got, _ = synth.super_walk_cpu(js, rows, missing)
    assert np.array_equal(helpers.bits(got), helpers.bits(want))
    # the tie rows sit on thresholds: a < read as <= would move some of them
    flipped = 0
    for t in trees[:8]:
        for r in tie[:300]:
            n = 0
            while t.left[n] != -1:
                x = r[t.feat[n]]
                if x == np.float32(t.cond[n]):
                    flipped += 1
                    break
                n = t.left[n] if x < np.float32(t.cond[n]) else t.right[n]
    assert ntree < 2 or flipped > 0


def test_fused_thresholds_sit_on_engineered_values():
    """fields_booster draws every threshold from the slab's engineered rows (PL / 100 and the 2-D broadcast included)
    or a float32 neighbour: rows of the slab hold thresholds of their feature exactly, PL among them."""
    grid = synth.GRIDS["C12"]
    pl, tropp, fields = helpers.synth_state(grid)
    k1, k2 = O.k_slab(pl, tropp, True, 4000.0)
    rows = S.engineered_rows(fields, k1, k2)
    js, trees = S.fields_booster(5, 40, rows)
    by_feature = S.thresholds_by_feature(trees)
    hits = np.zeros(len(rows), dtype=bool)
    hit_features = set()
    for f in range(S.NFEAT):
        on = np.isin(rows[:, f], np.array(sorted(by_feature[f]), dtype=np.float32))
        if on.any():
            hit_features.add(f)
        hits |= on
    assert hits.sum() >= 40 and 1 in hit_features and len(hit_features) >= 20, (hits.sum(), hit_features)
    # the PL thresholds are the float32 quotients, not the Pa values
    pa = set(float(x) for x in np.unique(pl))
    assert not (by_feature[1] & pa)
    # is2d features: values broadcast from the 2-D field
    for f in (0, 21, 22, 26):
        assert by_feature[f] and by_feature[f] <= set(float(v) for v in np.unique(np.nextafter(fields[f], np.float32(np.inf)))) | \
            set(float(v) for v in np.unique(fields[f])) | set(float(v) for v in np.unique(np.nextafter(fields[f], np.float32(-np.inf))))
