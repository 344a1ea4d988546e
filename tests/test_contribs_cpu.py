"""Per-feature contributions on the CPU: the test-support restatement (csrc/contribs_host.cpp, xgboost 1.6.0's
recursive TreeShap and CalculateContributionsApprox in float) against a float64 brute-force Shapley reference on
random boosters, local accuracy in both modes, and the refusal of a model without cover statistics."""
import json

import numpy as np
import pytest

from quickchem_amd import synth
from tests import booster_shapes as S
from tests import contribs_support as cs
from tests import helpers


@pytest.mark.parametrize("ntree,nfeat,depth,p_leaf", cs.CASES)
def test_exact_restatement_matches_brute_force(ntree, nfeat, depth, p_leaf):
    rng = np.random.default_rng(7000 + ntree * 100 + nfeat)
    js, trees, base = cs.random_booster(rng, ntree, nfeat, depth, p_leaf)
    rows = cs.random_rows(rng, 40 if nfeat >= 8 else 120, nfeat)
    for missing in (-999.0, float("nan")):
        got = synth.contribs_cpu(js, rows, nfeat, missing=missing)
        ref = cs.brute_force(trees, base, rows, missing, nfeat)
        assert cs.within(got, ref) <= 1.0, missing
    if nfeat > 2:   # fewer matrix columns than features: the absent ones are missing
        got = synth.contribs_cpu(js, rows[:, :nfeat - 2], nfeat, missing=-999.0)
        ref = cs.brute_force(trees, base, rows[:, :nfeat - 2], -999.0, nfeat)
        assert cs.within(got, ref) <= 1.0


def test_ties_and_signed_zeros_go_right():
    """x == cond goes right, -0.0 == +0.0: one split on feature 0 at 0.0, rows exactly on it."""
    rng = np.random.default_rng(3)
    js, trees, base = cs.random_booster(rng, 1, 2, 1, 0.0)
    trees[0]["cond"][0] = 0.0
    doc = json.loads(js)
    doc["learner"]["gradient_booster"]["model"]["trees"][0]["split_conditions"][0] = 0.0
    doc["learner"]["gradient_booster"]["model"]["trees"][0]["split_indices"][0] = 0
    trees[0]["feat"][0] = 0
    js = json.dumps(doc).encode()
    rows = np.array([[0.0, 1.0], [-0.0, 1.0], [1e-45, 1.0], [-1e-45, 1.0]], dtype=np.float32)
    got = synth.contribs_cpu(js, rows, 2, missing=float("nan"))
    ref = cs.brute_force(trees, base, rows, float("nan"), 2)
    assert cs.within(got, ref) <= 1.0
    assert got[0, 0] == got[1, 0] == got[2, 0] and got[3, 0] != got[0, 0]


@pytest.mark.parametrize("approximate", [False, True])
def test_local_accuracy(approximate):
    rng = np.random.default_rng(11)
    js, trees, base = cs.random_booster(rng, 30, 9, 8, 0.2)
    rows = cs.random_rows(rng, 500, 9)
    binary = synth.convert_model(js, "binary")
    for ntree_limit in (0, 7):
        got = synth.contribs_cpu(js, rows, 9, missing=-999.0, approximate=approximate, ntree_limit=ntree_limit)
        margin = helpers.oracle_predict(binary, rows, -999.0, option_mask=1, ntree_limit=ntree_limit)
        total = got.astype(np.float64).sum(axis=1)
        scale = 1.0 + np.abs(got.astype(np.float64)).sum(axis=1)
        assert np.all(np.abs(total - margin) <= 1e-5 * scale)


def test_approximate_restatement_is_the_saabas_walk():
    """Approximate mode against a float64 restatement of the definition: along the row's path, mean(next) -
    mean(current) into the split feature, means from the covers."""
    rng = np.random.default_rng(12)
    js, trees, base = cs.random_booster(rng, 10, 6, 7, 0.2)
    rows = cs.random_rows(rng, 200, 6)
    got = synth.contribs_cpu(js, rows, 6, missing=-999.0, approximate=True)
    ref = cs.saabas64(trees, base, rows, -999.0, 6)
    assert cs.within(got, ref) <= 1.0


def test_restatement_refuses_a_model_without_cover():
    rng = np.random.default_rng(5)
    js, _, _ = cs.random_booster(rng, 3, 4, 4, 0.1)
    doc = json.loads(js)
    for t in doc["learner"]["gradient_booster"]["model"]["trees"]:
        t["sum_hessian"] = [0.0] * len(t["sum_hessian"])
    rows = cs.random_rows(rng, 4, 4)
    with pytest.raises(Exception, match="no cover statistics"):
        synth.contribs_cpu(json.dumps(doc).encode(), rows, 4)


def test_path_table_of_a_small_booster():
    """Every leaf below a split is one path; a path's length is its distinct features."""
    rng = np.random.default_rng(6)
    js, trees, _ = cs.random_booster(rng, 5, 3, 6, 0.2)
    st = synth.contribs_table_stats(js)
    leaves = sum(sum(1 for l in t["left"] if l == -1) for t in trees if t["left"][0] != -1)
    assert st["paths"] == leaves and 1 <= st["max_len"] <= 3
    assert st["bytes"] == 16 * (st["paths"] + st["elements"]) + 4 * 8 * len(trees)


def test_paths_over_32_distinct_features_are_refused():
    """The exact kernels unroll a path's recurrences to at most 32 distinct features; 33 is refused, 32 is not."""
    rng = np.random.default_rng(8)
    js, _, _ = cs.caterpillar_booster(rng, 2, 40, 32)
    assert synth.contribs_table_stats(js)["max_len"] == 32
    js, _, _ = cs.caterpillar_booster(rng, 2, 40, 33)
    with pytest.raises(Exception, match="at most 32"):
        synth.contribs_table_stats(js)


@pytest.mark.parametrize("ntree,nfeat,depth,p_leaf", cs.CASES)
def test_float64_path_reference_matches_brute_force(ntree, nfeat, depth, p_leaf):
    """The float64 per-path TreeSHAP the GPU tests use where the brute force cannot go (40 features) is the Shapley
    sum itself, to float64 rounding."""
    rng = np.random.default_rng(7000 + ntree * 100 + nfeat)
    js, trees, base = cs.random_booster(rng, ntree, nfeat, depth, p_leaf)
    rows = cs.random_rows(rng, 40, nfeat)
    for missing in (-999.0, float("nan")):
        assert np.max(np.abs(cs.treeshap64(trees, base, rows, missing, nfeat) -
                             cs.brute_force(trees, base, rows, missing, nfeat))) < 1e-12


def test_float32_error_grows_with_path_length():
    """Why the 32-feature paths get a wider bound than 1e-5 (test_gpu_contribs.py::test_exact_on_long_paths): xgboost
    1.6.0's own recursive algorithm in float32 (the CPU restatement) misses 1e-5 * (1 + sum |phi|) against float64 on
    them; on depth-18 paths of the OH recipe it meets it."""
    rng = np.random.default_rng(41)
    js, trees, base = cs.caterpillar_booster(rng, 24, 40, 32)
    rows = rng.normal(0, 1.0, (1000, 40)).astype(np.float32)
    rows[rng.random(rows.shape) < 0.02] = np.nan
    err = cs.within(synth.contribs_cpu(js, rows, 40, missing=-999.0), cs.treeshap64(trees, base, rows, -999.0, 40))
    assert 1.0 < err < 10.0


# ---- launch shapes (csrc/contribs.cpp plan_contribs, exposed as synth.contribs_plan) ----

def test_plan_at_its_boundaries():
    """(split, groups, trees_per_group, direct_launches) at every edge of the plan: 4 096 tiles split, 4 097 do not;
    a `part` of exactly 1 GiB splits, one tile more does not; 8 192 direct tiles are one launch, 8 193 two; fewer than
    two trees, and "ohx_contribs_split" = off, never split."""
    tile = 64
    assert synth.contribs_plan(4096 * tile, 8, 10) == (True, 2, 5, 0)
    assert synth.contribs_plan(4096 * tile + 1, 8, 10) == (False, 0, 0, 1)
    # part = tiles * ntree * F * 64 floats: 2 048 tiles x 16 trees x 128 features x 64 x 4 B = 1 GiB exactly
    assert 2048 * 16 * 128 * tile * 4 == 1 << 30
    assert synth.contribs_plan(2048 * tile, 128, 16) == (True, 4, 4, 0)
    assert synth.contribs_plan(2048 * tile + 1, 128, 16) == (False, 0, 0, 1)
    assert synth.contribs_plan(8192 * tile, 8, 3) == (False, 0, 0, 1)
    assert synth.contribs_plan(8192 * tile + 1, 8, 3) == (False, 0, 0, 2)
    assert synth.contribs_plan(3 * 8192 * tile, 8, 3) == (False, 0, 0, 3)
    for ntree in (0, 1):
        assert synth.contribs_plan(64, 27, ntree) == (False, 0, 0, 1)
    assert synth.contribs_plan(64, 27, 2) == (True, 2, 1, 0)
    assert synth.contribs_plan(64, 27, 100, allow_split=False) == (False, 0, 0, 1)
    assert synth.contribs_plan(0, 27, 100) == (False, 0, 0, 0)
    # groups fill the chip's 8 192 wave slots: ceil(8192 / tiles) of them, at most one per tree
    assert synth.contribs_plan(100 * tile, 27, 135) == (True, 68, 2, 0)
    assert synth.contribs_plan(1, 27, 135) == (True, 135, 1, 0)


# ---- the adversarial boosters (tests/booster_shapes.py contribs_booster) ----

def _base(js):
    return float(np.float32(json.loads(js)["learner"]["learner_model_param"]["base_score"]))


@pytest.mark.parametrize("ntree", [1, 2, 3, 5, 10])
def test_restatement_on_adversarial_boosters(ntree):
    """xgboost 1.6.0's recursive algorithm in float32 against float64 per-path TreeSHAP on chains of up to 27 distinct
    features with repeats, 1 / 1000 leaf covers, thresholds on +-0, denormals and +-3e38, and rows half of which sit on
    a threshold or one float32 step from it, for -999, NaN, +inf and -inf as the missing marker.  Where paths stay
    within 18 distinct features it meets 1e-5 (1 + sum |phi|).  Beyond, 1.6.0's unwinding of a repeated feature
    (unwind_path: the extend recurrence run backwards, dividing by the fractions) loses float32 precision by up to
    three orders of magnitude - the GPU tests bound the kernels by this error, and the float64 reference here keeps
    local accuracy to the float32 margin's rounding."""
    js, trees = S.contribs_booster(3000 + ntree, ntree)
    base, d = _base(js), cs.tree_dicts(trees)
    long_paths = synth.contribs_table_stats(js)["max_len"] > 18
    binary = synth.convert_model(js, "binary")
    for missing in (-999.0, float("nan"), float("inf"), float("-inf")):
        rows = S.rows_for(ntree * 10 + 1, trees, 512, missing)
        ref = cs.treeshap64(d, base, rows, missing, S.NFEAT)
        got = synth.contribs_cpu(js, rows, S.NFEAT, missing=missing)
        assert np.all(np.isfinite(got))
        err = cs.within(got, ref)
        assert err <= (2000.0 if long_paths else 1.0), (missing, err)
        margin = helpers.oracle_predict(binary, rows, missing, option_mask=1)
        assert np.all(np.abs(ref.sum(axis=1) - margin) <= 1e-6 * (1.0 + np.abs(ref).sum(axis=1))), missing
        # approximate mode: the Saabas walk in float64
        approx = synth.contribs_cpu(js, rows[:128], S.NFEAT, missing=missing, approximate=True)
        assert cs.within(approx, cs.saabas64(d, base, rows[:128], missing, S.NFEAT)) <= 1.0, missing


def test_adversarial_boosters_reach_the_long_length_classes():
    """The 10- and 135-tree boosters hold paths of 25 - 27 and of 21 - 24 distinct features (the 32- and 24-feature
    length classes of the exact kernels), each with a feature split on twice."""
    for ntree in (10, 135):
        js, trees = S.contribs_booster(3000 + ntree, ntree)
        lens = [x for t in trees for x in S.distinct_path_lengths(t)]
        assert any(25 <= n <= 27 and rep for n, rep in lens), ntree
        assert any(21 <= n <= 24 and rep for n, rep in lens), ntree
        assert synth.contribs_table_stats(js)["max_len"] == max(n for n, _ in lens)


def test_treeshap64_with_zero_cover_leaves_is_the_shapley_value():
    """A leaf of cover 0 gives a zero fraction of exactly 0; the float64 reference then matches the brute force."""
    rng = np.random.default_rng(17)
    js, trees, base = cs.random_booster(rng, 6, 8, 7, 0.2, zero_leaves=0.3)
    assert sum(c == 0.0 for t in trees for c in t["cover"]) > 10
    rows = cs.random_rows(rng, 60, 8)
    for missing in (-999.0, float("nan")):
        ref = cs.brute_force(trees, base, rows, missing, 8)
        assert np.max(np.abs(cs.treeshap64(trees, base, rows, missing, 8) - ref)) < 1e-12
        assert np.max(np.abs(cs.treeshap64(trees, base, rows[:, :5], missing, 8) -
                             cs.brute_force(trees, base, rows[:, :5], missing, 8))) < 1e-12


def test_restatement_with_zero_cover_leaves():
    """What xgboost 1.6.0's algorithm gives where a zero fraction is 0: its unwound sum skips an element with one and
    zero fraction both 0 (the branch beside the division by the zero fraction), and zero fractions of 0 only reach
    leaves - a split's cover must be > 0, and a feature is unwound only at a split below it - so the division never
    meets a 0 and the result is finite, and the Shapley value."""
    rng = np.random.default_rng(17)
    js, trees, base = cs.random_booster(rng, 6, 8, 7, 0.2, zero_leaves=0.3)
    rows = cs.random_rows(rng, 60, 8)
    for missing in (-999.0, float("nan")):
        got = synth.contribs_cpu(js, rows, 8, missing=missing)
        assert np.all(np.isfinite(got))
        assert cs.within(got, cs.brute_force(trees, base, rows, missing, 8)) <= 1.0
        approx = synth.contribs_cpu(js, rows, 8, missing=missing, approximate=True)
        assert cs.within(approx, cs.saabas64(trees, base, rows, missing, 8)) <= 1.0
    js27, t27 = S.contribs_booster(99, 10, zero_cover_leaves=True)
    assert sum(t.hess[n] == 0.0 for t in t27 for n in range(len(t.left)) if t.left[n] == -1) > 50
    assert np.all(np.isfinite(synth.contribs_cpu(js27, S.rows_for(5, t27, 256, -999.0), S.NFEAT, missing=-999.0)))
