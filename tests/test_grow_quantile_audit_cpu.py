"""Without a GPU: the audited quantile cases of tests/test_gpu_grow_quantile.py (grow_audit_support.Q_CASES) on the
restatement alone.  Every case's restated trees pass the exact audit (every check but `leaf`, which a quantile tree does not
meet by design) and the leaf check written for them (grow_audit_support.quantile_leaf_violations), and the conditions under
which both have something to say hold before the GPU is asked: at least 10 decided split nodes a call, at least 95 % of the
float32 records pinned, a level with a split beside a node that gamma closed under either setting with gamma > 0, a split that
min_child_weight moved, and in every sampled tree a leaf that holds a row out of the bag and one that holds a row of weight
0.  The counts are printed per case.  Then the leaf check and the audit report each planted error, at that leaf or node
alone.  Nothing here calls the library."""
import numpy as np
import pytest

from tests import grow_audit_support as A
from tests import grow_quantile_support as Q
from tests import grow_weighted_support as W
from tests.test_grow_audit_cpu import copy_of, leaves_below, resplit

F32 = np.float32


def test_the_table_covers_what_it_is_meant_to():
    cases = A.Q_CASES
    assert 10 <= len(cases) <= 14 and len(set(cases)) == len(cases)
    assert {c[2] for c in cases} == {0.05, 0.5, 0.95} and {c[0] for c in cases} == {"weighted", "sampled"}
    assert {c[3] for c in cases} == set(A.Q_SETTINGS)
    for setting in A.Q_SETTINGS:
        assert {c[1] for c in cases if c[3] == setting} == {"host", "device"}, setting
    for c in cases:
        kw = A.q_hyper(c)
        mant = np.frexp(kw["eta"])[0]
        assert mant == 0.5 and kw["eta"] in (1.0, 0.125, 0.03125), "a power of two: the multiply is inverted exactly"
        assert kw["rounds"] == 2 and kw["max_depth"] == 6
        assert (c[0] == "sampled") == (kw.get("subsample") == 0.5 and kw.get("colsample_bytree") == 0.5 and kw.get("seed") == 11)
    first, second = (A.Q_SETTINGS[k] for k in ("g0.5-l0.5-mcw8-eta1/32", "g2-l0-mcw40-eta1"))
    assert first == dict(gamma=0.5, reg_lambda=0.5, min_child_weight=8.0, eta=1.0 / 32) and A.Q_SETTINGS["lambda0.5"] == dict(reg_lambda=0.5)
    assert second == dict(gamma=2.0, reg_lambda=0.0, min_child_weight=40.0, eta=1.0)


@pytest.fixture(scope="module")
def reached():
    return {}


@pytest.mark.parametrize("case", A.Q_CASES, ids=A.q_id)
def test_a_case_passes_the_audit_and_leaves_it_enough_to_judge(case, reached):
    x, y, w, cuts, _, want = A.q_restated(case)
    *_, plain = A.q_restated(case, dict(max_depth=A.Q_DEPTH))
    trees = want["all_trees"]
    assert len(trees) == 2 and any(not np.array_equal(a["value"], b["value"]) for a, b in zip(trees, plain["all_trees"])), "the setting changes a tree"
    audits = A.q_audits(case, x, y, w, cuts, trees)
    for r, (a, pred) in enumerate(audits):
        assert a.leaf_rule is None
        assert a.violations() == [], (case, r)
        assert A.quantile_leaf_violations(a, pred, y, case[2]) == [], (case, r)
        assert np.array_equal(pred.view(np.uint32), want["preds"][r].view(np.uint32)), "the margins of the round"
        # the audit's own walk against the restatement's pos, and its leaves against the keys the restatement set
        leaves = [p for p in a.order if trees[r]["left"][p] < 0]
        assert all(np.array_equal(np.sort(a.rows[p]), np.flatnonzero(want["pos"][r] == p)) for p in leaves)
        assert sorted(want["leaf_keys"][r]) == [p for p in sorted(leaves) if a.H[p] > 0]
    records, pinned = (sum(a.stats[k] for a, _ in audits) for k in ("records", "pinned"))
    decided = [A.decided(a) for a, _ in audits]
    got = A.q_reaches(case)
    reached[case] = got
    print(A.q_id(case), "leaves", [a.size // 2 + 1 for a, _ in audits], "decided", decided, "pinned %d of %d" % (pinned, records),
          "mixed level", got["mixed"], "moved split", got["moved"], "leaves with a row out of the bag", got["out_of_bag"],
          "leaves with a row of weight 0", got["weightless"])
    assert sum(decided) >= 10, "splits at which a wrong choice would be reported"
    assert pinned >= 0.95 * records, "the bounds pin nearly every float32 record to one value"
    assert all(n >= 1 for n in got["weightless"]), "a leaf that holds a row of weight 0"
    if case[0] == "sampled":
        assert all(n >= 1 for n in got["out_of_bag"]), "a leaf that holds a row out of the bag"
    else:
        assert got["out_of_bag"] == [0, 0]


def test_the_settings_reach_gamma_and_the_child_minimum(reached):
    """After the cases above (their profiles are shared): a level with a split beside a node that gamma closed under either
    setting with gamma > 0, and a split that min_child_weight moved."""
    got = {c: reached.get(c) or A.q_reaches(c) for c in A.Q_CASES}
    for setting, kw in A.Q_SETTINGS.items():
        if kw.get("gamma", 0.0) > 0:
            assert any(got[c]["mixed"] for c in A.Q_CASES if c[3] == setting), setting
        if kw.get("min_child_weight", 0.0) > 0:
            assert any(got[c]["moved"] for c in A.Q_CASES if c[3] == setting), setting


# ---- the leaf check bites ----

BAGGED = [c for c in A.Q_CASES if c[0] == "sampled" and c[3] == "g0.5-l0.5-mcw8-eta1/32" and c[2] == 0.05][0]


def sound(case):
    """-> per restated tree (a copy of the tree, the Audit's inputs, the Audit, the margins)."""
    x, y, w, cuts, _, want = A.q_restated(case)
    trees = want["all_trees"]
    out = []
    for r, (a, pred) in enumerate(A.q_audits(case, x, y, w, cuts, trees)):
        inputs = A.round_inputs(case[0], "pairs", A.q_hyper(case), x, y, w, cuts, trees, r, objective="quantile", quantile_alpha=case[2])
        out.append((copy_of(trees[r]), inputs, a, pred))
    return y, w, out


def leaf_report(tree, inputs, pred, y, alpha):
    return A.quantile_leaf_violations(A.Audit(tree=tree, **inputs), pred, y, alpha)


def counted(a, p):
    rows = a.rows[p]
    return rows[a.hq[rows] > 0]


def test_a_leaf_moved_to_the_next_key_among_its_rows_is_reported():
    y, w, trees = sound(BAGGED)
    tried = 0
    for tree, inputs, a, pred in trees:
        k = Q.keys(y - pred)
        for p in [p for p in a.order if tree["left"][p] < 0][:6]:
            mine = int(Q.keys(np.asarray([tree["value"][p] / a.eta], F32))[0])
            above = sorted(int(v) for v in set(k[counted(a, p)].tolist()) if v > mine)
            if not above:
                continue
            moved = copy_of(tree)
            moved["value"][p] = Q.leaf_value(above[0], a.eta)
            assert [v[:2] for v in leaf_report(moved, inputs, pred, y, BAGGED[2])] == [(p, "quantile_leaf")], p
            assert A.Audit(tree=moved, **inputs).violations() == [], "the other checks do not look at a leaf's value"
            tried += 1
    assert tried >= 6


def test_a_leaf_that_counts_rows_out_of_the_bag_or_rows_of_no_weight_is_reported():
    y, w, trees = sound(BAGGED)
    aq = Q.alpha_q(BAGGED[2])
    tried = {"bag": 0, "weight": 0}
    for tree, inputs, a, pred in trees:
        k = Q.keys(y - pred)
        everyone = np.asarray(inputs["hq"], np.uint64)                      # the pairs of every row, the bag not applied
        in_bag = np.asarray(inputs["in_bag"], bool)
        as_ones = np.where(in_bag & (everyone == 0), np.uint64(A.ONE), np.where(in_bag, everyone, np.uint64(0)))
        for p in [p for p in a.order if tree["left"][p] < 0]:
            rows = a.rows[p]
            mine = int(Q.keys(np.asarray([tree["value"][p] / a.eta], F32))[0])
            for what, hq in (("bag", everyone), ("weight", as_ones)):
                other = Q.leaf_key_fast(k[rows], hq[rows], aq)
                if other == mine:
                    continue
                wrong = copy_of(tree)
                wrong["value"][p] = Q.leaf_value(other, a.eta)
                assert [v[:2] for v in leaf_report(wrong, inputs, pred, y, BAGGED[2])] == [(p, "quantile_leaf")], (what, p)
                tried[what] += 1
    assert tried["bag"] >= 6 and tried["weight"] >= 6, tried


@pytest.mark.parametrize("alpha,step", ((0.5, 1), ((2.0 ** 23 + 1) / 2.0 ** 24, -1)))
def test_a_leaf_at_an_alpha_q_one_off_is_reported_where_that_crosses_a_row(alpha, step):
    """Two rows of weight 1: at alpha_q = 2^23 the rule holds at the lower with equality, at 2^23 + 1 only at the upper."""
    aq = Q.alpha_q(alpha)
    assert aq == (1 << 23) + (step < 0)
    r, hq = np.asarray([-1.5, 2.25], F32), W.hess_fixed(np.ones(2, F32))
    right, off = (Q.leaf_key(Q.keys(r), hq, q) for q in (aq, aq + step))
    assert right != off and {right, off} == set(int(v) for v in Q.keys(r))
    for eta in (1.0, 0.125, 0.03125):
        assert A.quantile_leaf_verdict(Q.leaf_value(right, eta), 0.0, eta, r, hq, aq) is None
        assert "quantile" in A.quantile_leaf_verdict(Q.leaf_value(off, eta), 0.0, eta, r, hq, aq)


def test_a_value_that_is_no_rows_residual_a_denormal_and_a_weightless_leaf():
    y, w, trees = sound(BAGGED)
    for tree, inputs, a, pred in trees:
        p = [p for p in a.order if tree["left"][p] < 0][1]
        for v in (np.nextafter(tree["value"][p], F32(np.inf)), np.nextafter(tree["value"][p], F32(-np.inf)), tree["base_weight"][p] * a.eta):
            wrong = copy_of(tree)
            wrong["value"][p] = v
            found = leaf_report(wrong, inputs, pred, y, BAGGED[2])
            assert [f[:2] for f in found] == [(p, "quantile_leaf")] and "no row" in found[0][2], found
    assert "denormal" in A.quantile_leaf_verdict(F32(2.0 ** -130), 0.0, 0.125, np.asarray([2.0 ** -127], F32), [A.ONE], 1 << 23)
    # a leaf without a row that counts keeps the split kernel's value, and nothing else
    none = np.zeros(0, F32)
    assert A.quantile_leaf_verdict(F32(0.75) * F32(0.125), F32(0.75), 0.125, none, none.astype(np.uint64), 1 << 23) is None
    assert "without weight" in A.quantile_leaf_verdict(F32(0.5), F32(0.75), 0.125, none, none.astype(np.uint64), 1 << 23)
    # -0.0 is no value of a leaf: the header's key of a zero is that of +0.0
    zeros = np.asarray([-0.0, 0.0], F32)
    assert A.quantile_leaf_verdict(F32(0.0), 0.0, 1.0, zeros, [A.ONE, A.ONE], 1 << 23) is None
    assert A.quantile_leaf_verdict(F32(-0.0), 0.0, 1.0, zeros, [A.ONE, A.ONE], 1 << 23) is not None


def test_the_leaf_keyword_leaves_out_the_leaf_check_and_nothing_else():
    y, w, trees = sound(BAGGED)
    for tree, inputs, a, pred in trees:
        assert inputs["leaf"] is None
        newton = A.Audit(tree=tree, **dict(inputs, leaf="newton")).violations()
        leaves = sorted(p for p in a.order if tree["left"][p] < 0)
        assert newton and {v[1] for v in newton} == {"leaf"} and {v[0] for v in newton} <= set(leaves)
        assert len(newton) > len(leaves) // 2, "a quantile leaf is no Newton step"
        off = copy_of(tree)
        off["loss_chg"][0] = -off["loss_chg"][0]
        off["sum_hess"][leaves[0]] += F32(1.0)
        assert [v[:2] for v in A.Audit(tree=off, **inputs).violations()] == [(0, "loss_chg"), (leaves[0], "sum_hess")]


def test_a_decided_split_swapped_for_its_runner_up_is_reported():
    tried = 0
    for case in (BAGGED, A.Q_CASES[1]):
        y, w, trees = sound(case)
        for tree, inputs, a, pred in trees:
            for p in a.order:
                if not leaves_below(tree, p):
                    continue
                ranked = a.ranked(p)
                if len(ranked) < 2 or tuple(ranked[0][2:]) != a.split_of(p) or not ranked[0][0] - ranked[1][0] > ranked[0][1] + ranked[1][1]:
                    continue                       # (a tie within the bounds is not judged)
                if not ranked[1][0] - ranked[1][1] > a.gammaF:
                    continue                       # (a runner-up that gamma would close is another error)
                found = A.Audit(tree=resplit(tree, inputs, a, p, *ranked[1][2:]), **inputs).violations()
                children = (int(tree["left"][p]), int(tree["right"][p]))
                assert [v[:2] for v in found if v[0] == p] == [(p, "optimality")], (p, found)
                # (a child of the other split holds other rows, and may have a candidate above gamma that the leaf it is does not take)
                assert all(v[0] in children and v[1] == "closure" for v in found if v[0] != p), (p, found)
                tried += 1
    assert tried >= 6
