"""Without a GPU: the cases of tests/test_gpu_grow_hyper.py on the restatements alone, and the exact audit of
tests/grow_audit_support.py.  Every case asserts what its setting is meant to reach, its restated trees pass the audit with
no violation, and the restatement's own doubles stay inside the derived bounds: over all cases the largest error seen is 0.09
of the bound for the loss_chg of a split and 0.31 for the child weights of a constrained split, and the bounds pin 11217 of
11219 float32 records to a single value.  The audit reports each of five planted errors at the node that holds it.  Nothing
here calls the library."""
from fractions import Fraction

import numpy as np
import pytest

from tests import grow_audit_support as A
from tests import grow_objective_support as O
from tests import grow_reg_support as RG
from tests import grow_support as G

F32 = np.float32


def test_the_cases_cover_every_policy_at_every_setting_and_every_kind_in_both_forms():
    have = {(p.replace("constrained_regularised", "constrained"), s) for _, _, p, s, _ in A.CASES}
    for policy in ("pairs", "regularised", "constrained"):
        for setting in A.SETTINGS:
            if setting == "lambda0" and policy == "pairs":
                continue                        # (refused: see grow_audit_support.CASES)
            assert (policy, setting) in have, (policy, setting)
    assert {(k, f) for k, f, *_ in A.CASES} == {(k, f) for k in A.ROWS for f in ("host", "device")}
    assert {p for _, _, p, *_ in A.CASES} == set(A.POLICIES)
    assert all(("deep" in k) == (A.hyper(k, s)["max_depth"] == 10) and (s != "deep_combination" or "deep" in k) for k, _, _, s, _ in A.CASES)
    assert {(c[0], c[2]) for c in A.AUDITED} == {(k, p) for k in ("weighted", "deep") for p in ("pairs", "regularised", "constrained")}


@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
def test_a_case_reaches_its_setting_and_its_restated_trees_pass_the_audit(case):
    kind, _, policy, setting, seed = case
    want = A.reaches(kind, policy, setting, seed)
    x, y, w, cuts, _, _ = A.restated(kind, policy, setting, seed)
    seen = A.profile(kind, policy, setting, seed)
    for r, a in enumerate(A.audits(kind, policy, setting, x, y, w, cuts, want["all_trees"])):
        assert a.violations() == [], (case, r)
        assert a.stats["records"] == a.size + a.size // 2, "a base_weight a node and a loss_chg a split"
        assert a.stats["pinned"] >= 0.99 * a.stats["records"], "the bounds pin nearly every float32 record to one value"
        if A.POLICIES[policy][2]:
            assert A.sweep_violations(want["all_trees"][r], x, cuts, A.CONSTRAINTS) == 0, (case, r)
        # the restatement's own doubles against the exact values, as a fraction of the derived bounds
        worst = {"loss_chg": 0.0, "weight": 0.0}
        for p in a.order:
            if want["all_trees"][r]["left"][p] >= 0:
                best = seen[r][p]["best"]
                assert best[1:4] == a.split_of(p)
                cand = [c for c in a.candidates(p) if c[1:4] == best[1:4]][0]
                loss, e = a.loss(p, cand)
                worst["loss_chg"] = max(worst["loss_chg"], float(abs(Fraction(best[0]) - loss)) / e)
                if A.POLICIES[policy][2]:
                    for double, exact, bound in ((best[6], cand[6], cand[7]), (best[7], cand[8], cand[9])):
                        if double != exact[0] / exact[1]:
                            worst["weight"] = max(worst["weight"], float(abs(Fraction(double) - Fraction(*exact))) / bound)
        print(A.case_id(case), "tree", r, "the restatement's error / bound:", worst, a.stats)
        assert worst["loss_chg"] < 1 and worst["weight"] < 1, "the reference inside the derived bounds"


def test_a_free_tree_is_not_monotone():
    """The free twins of the constrained cases that the GPU tests audit: the sweep bites."""
    for kind, _, policy, setting, seed in A.AUDITED:
        if policy == "pairs":
            x, _, _, cuts, _, want = A.restated(kind, policy, setting, seed)
            assert all(A.sweep_violations(t, x, cuts, A.CONSTRAINTS) > 0 for t in want["all_trees"]), kind


@pytest.mark.parametrize("kind", tuple(A.ROWS))
def test_lambda_0_without_a_step_is_refused_and_with_a_step_is_not(kind):
    """The restatement of what tests/test_gpu_grow_hyper.py asks of the library: at lambda 0 a child of hessian sum near 1e-5
    gets a leaf that throws a margin out of range, and "label" refuses the call; a step of 0.5 bounds every leaf."""
    kw = A.hyper(kind, dict(reg_lambda=0.0))
    common = dict(bins=A.BINS, nfeat=A.NFEAT, rounds=2, held_out=A.HELD, lam=0.0, subsample=kw.get("subsample", 1.0),
                  colsample=kw.get("colsample_bytree", 1.0), draw_seed=kw.get("seed", 0))
    with pytest.raises(ValueError, match="^label: a residual is not finite or reaches 256"):
        O.restated("pseudohuber", A.SLOPE, A.ROWS[kind], A.SEED, kw["max_depth"], **common)
    *_, want = RG.restated("pseudohuber", A.SLOPE, 0.0, 0.5, "rmse", A.ROWS[kind], A.SEED, kw["max_depth"], **common)
    assert want["nodes_added"] > 100 and (kind != "weighted" or want["nodes_added"] == 172)
    q, hq = O.pairs("pseudohuber", A.SLOPE, np.full(A.ROWS[kind], O.BASE, F32), *O.inputs(A.ROWS[kind], A.SEED, A.NFEAT, A.BINS, 0)[1:3])
    assert 0 < int(hq[hq > 0].min()) * 2.0 ** -24 < 1e-4, "hessians this small"


# ---- the audit can fail ----

KIND, POLICY, SETTING, CASE_SEED, TREE = "weighted", "constrained", "combination", 284, 1


@pytest.fixture(scope="module")
def sound():
    """-> (the second restated tree of a constrained case, what it was grown on, its audit)."""
    return sound_tree(TREE)


def sound_tree(r):
    x, y, w, cuts, _, want = A.restated(KIND, POLICY, SETTING, CASE_SEED)
    trees = want["all_trees"]
    inputs = A.round_inputs(KIND, POLICY, SETTING, x, y, w, cuts, trees, r)
    tree = {k: trees[r][k] for k in G.ARRAYS}
    a = A.Audit(tree=tree, **inputs)
    assert a.violations() == []
    return tree, inputs, a


def copy_of(tree):
    return {k: v.copy() for k, v in tree.items()}


def audit(tree, inputs):
    return A.Audit(tree=tree, **inputs).violations()


def split_nodes(tree, a, leaves_below=False):
    out = [p for p in a.order if tree["left"][p] >= 0]
    if leaves_below:
        out = [p for p in out if tree["left"][tree["left"][p]] < 0 and tree["left"][tree["right"][p]] < 0]
    return out


def test_the_audit_reports_a_split_moved_to_the_second_best_candidate(sound):
    tree, inputs, a = sound
    cut_ptr, cut_values = inputs["cuts"]
    tried = 0
    for p in split_nodes(tree, a, leaves_below=True):
        ranked = a.ranked(p)
        (loss, e, *key), (loss2, e2, f, j, dl) = ranked[0], ranked[1]
        assert tuple(key) == (int(tree["feature"][p]), a.j[p], int(tree["default_left"][p])), "the split is the best candidate"
        if not loss - loss2 > e + e2:
            continue                           # (a tie within the bounds is not judged)
        t = copy_of(tree)
        t["feature"][p], t["default_left"][p], t["value"][p] = f, dl, cut_values[int(cut_ptr[f]) + j]
        found = audit(t, inputs)
        assert (p, "optimality") in {v[:2] for v in found}, (p, found)
        assert {v[0] for v in found} <= {p, int(tree["left"][p]), int(tree["right"][p])}, found
        tried += 1
    assert tried >= 3


def test_the_audit_reports_a_changed_feature(sound):
    tree, inputs, a = sound
    p = split_nodes(tree, a)[2]
    t = copy_of(tree)
    t["feature"][p] = (int(t["feature"][p]) + 1) % A.NFEAT
    found = audit(t, inputs)
    assert (p, "structure") in {v[:2] for v in found} and all(v[1] == "structure" for v in found), found


def test_the_audit_reports_a_base_weight_two_ulps_off(sound):
    tree, inputs, a = sound
    for p in split_nodes(tree, a)[:4] + [a.order[-1]]:
        for towards in (np.inf, -np.inf):
            t = copy_of(tree)
            t["base_weight"][p] = np.nextafter(np.nextafter(t["base_weight"][p], F32(towards)), F32(towards))
            found = audit(t, inputs)
            want = [(p, "base_weight")] + ([(p, "leaf")] if tree["left"][p] < 0 else [])
            assert [v[:2] for v in found] == want, (p, found)


def test_the_audit_reports_a_loss_chg_of_the_wrong_sign(sound):
    tree, inputs, a = sound
    for p in split_nodes(tree, a)[:4]:
        t = copy_of(tree)
        t["loss_chg"][p] = -t["loss_chg"][p]
        assert [v[:2] for v in audit(t, inputs)] == [(p, "loss_chg")]


def test_the_audit_reports_a_constrained_child_moved_across_mid(sound):
    tree, inputs, a = sound
    moved = 0
    for p in split_nodes(tree, a):
        l, r = int(tree["left"][p]), int(tree["right"][p])
        if A.CONSTRAINTS[int(tree["feature"][p])] == 0 or tree["base_weight"][l] == tree["base_weight"][r]:
            continue
        for c, other in ((l, r), (r, l)):
            t = copy_of(tree)
            t["base_weight"][c] = t["base_weight"][other]         # the sibling's weight lies beyond mid
            if t["left"][c] < 0:
                t["value"][c] = t["base_weight"][c] * F32(inputs["eta"])
            assert [v[:2] for v in audit(t, inputs)] == [(c, "base_weight")], (p, c)
            moved += 1
    assert moved >= 6


def test_the_audit_reports_a_split_below_gamma():
    """A node that gamma closed is given the split its best candidate would give, its children's records as the header makes
    them; and the same node, left closed under a gamma of 0, is reported as wrongly closed.  (The first tree of the case:
    gamma closes no node of the second.)"""
    tree, inputs, a = sound_tree(0)
    cut_ptr, cut_values = inputs["cuts"]
    closed = [p for p in a.order if tree["left"][p] < 0 and a.evaluated(p) and a.candidates(p)]
    assert closed, "gamma closes a node with an admitted candidate"
    for p in closed:
        loss, e, f, j, dl = a.ranked(p)[0]
        assert loss <= a.gammaF
        cand = [c for c in a.candidates(p) if c[1:4] == (f, j, dl)][0]
        GL, HL, wL, wR = cand[4], cand[5], cand[6], cand[8]
        k = len(tree["left"])
        t = {key: np.concatenate([v, np.zeros(2, v.dtype)]) for key, v in tree.items()}
        t["left"][p], t["right"][p], t["feature"][p], t["default_left"][p] = k, k + 1, f, dl
        t["value"][p], t["loss_chg"][p] = cut_values[int(cut_ptr[f]) + j], F32(float(loss))
        for c, Gs, H, w in ((k, GL, HL, wL), (k + 1, a.G[p] - GL, a.H[p] - HL, wR)):
            t["left"][c] = t["right"][c] = -1
            t["parent"][c] = p + (G.LEFT_BIT if c == k else 0)
            t["sum_hess"][c], t["base_weight"][c] = F32(float(H) * 2.0 ** -24), F32(w[0] / w[1])
            t["value"][c] = t["base_weight"][c] * F32(inputs["eta"])
        assert [v[:2] for v in audit(t, inputs)] == [(p, "gamma")], p
    assert any(a.ranked(p)[0][0] > a.ranked(p)[0][1] for p in closed), "a best candidate between 0 and gamma"
    found = A.Audit(tree=copy_of(tree), **dict(inputs, gamma=0.0)).violations()
    assert {v[:2] for v in found} == {(p, "closure") for p in closed if a.ranked(p)[0][0] > a.ranked(p)[0][1]}, found
