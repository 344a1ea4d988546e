"""Per-feature contributions on the CPU: the test-support restatement (csrc/contribs_host.cpp, xgboost 1.6.0's
recursive TreeShap and CalculateContributionsApprox in float) against a float64 brute-force Shapley reference on
random boosters, local accuracy in both modes, and the refusal of a model without cover statistics."""
import json

import numpy as np
import pytest

from quickchem_amd import synth
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

    def means(t):
        m = [0.0] * len(t["left"])

        def fill(n):
            if t["left"][n] == -1:
                m[n] = float(np.float32(t["cond"][n]))
            else:
                l, r = t["left"][n], t["right"][n]
                m[n] = (fill(l) * t["cover"][l] + fill(r) * t["cover"][r]) / t["cover"][n]
            return m[n]
        fill(0)
        return m
    ref = np.zeros((len(rows), 7))
    for t in trees:
        m = means(t)
        for r, x in enumerate(rows):
            ref[r, 6] += m[0]
            n = 0
            while t["left"][n] != -1:
                f = t["feat"][n]
                miss = np.isnan(x[f]) or x[f] == -999.0
                nxt = (t["left"][n] if t["dl"][n] else t["right"][n]) if miss else \
                    (t["left"][n] if x[f] < np.float32(t["cond"][n]) else t["right"][n])
                ref[r, f] += m[nxt] - m[n]
                n = nxt
    ref[:, 6] += base
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
