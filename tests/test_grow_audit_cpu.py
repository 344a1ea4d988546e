"""Without a GPU: the cases of tests/test_gpu_grow_audit.py on the restatements alone.  Every case of INLINE_CASES,
COLSAMPLE_CASES and AUDITED_MORE (tests/grow_audit_support.py) asserts what its setting is meant to reach, its restated trees
pass the exact audit with no violation, and the conditions under which the audit has something to say hold before the GPU
is asked: at least 10 split nodes in every audited tree, at least 10 `decided` split nodes an audited call, at least 95 % of
the float32 records of a case pinned to a single value, and the restatement's own doubles below 1 of the derived bounds.  The
pinned share and the decided counts are printed per case.  The audit reports each of seven planted errors that it newly
claims to see, and a callable `kept` that takes nothing away gives the verdicts of the list.  Nothing here calls the
library."""
from fractions import Fraction

import numpy as np
import pytest

from tests import grow_audit_support as A
from tests import grow_colsample_support as K
from tests import grow_sampled_support as P
from tests import grow_support as G

F32 = np.float32
EVERY_CASE = tuple(dict.fromkeys(A.INLINE_CASES + A.COLSAMPLE_CASES + A.AUDITED_MORE))


def test_the_tables_cover_what_they_are_meant_to():
    inline, cols = A.INLINE_CASES, A.COLSAMPLE_CASES
    assert all(c[2:4] == ("squarederror", "pairs") and c[6] == A.NO_FRACTIONS for c in inline)
    assert {(c[0], c[1]) for c in inline} == {(k, f) for k in A.INLINE_KINDS for f in ("host", "device")}
    for setting in A.SETTINGS_MORE:
        if setting == "deep_combination":
            assert {c[0] for c in inline if c[4] == setting} == {"deep", "deep_sampled"}
        else:
            assert {c[0] in A.COUNT_KINDS for c in inline if c[4] == setting} == {True, False}, setting
    assert all(A.case_hyper(c)["max_depth"] <= 8 for c in inline if c[0] in A.COUNT_KINDS)
    assert [A.case_hyper(c)["min_child_rows"] for c in inline if c[0] == "plain" and c[4] in ("mcw8", "combination")] == [8, 3]
    assert any(A.case_hyper(c)["min_child_rows"] == 40 for c in inline)
    assert all((c[0], A.case_hyper(c)["max_depth"]) in (("sampled", 6), ("deep_sampled", 10)) and max(c[6]) < 1 for c in cols)
    assert all(A.nfeat_of(c) == (4 if A.POLICIES[c[3]][2] else 8) for c in cols)
    assert {c[3] for c in cols if c[2] == "pseudohuber" and "combination" in c[4]} == set(A.POLICIES)
    assert sorted(c[0] for c in cols if c[2] == "squarederror") == ["deep_sampled", "sampled"]
    assert [c[4] for c in cols].count("gamma2") == 1 and [c[4] for c in cols].count("mcw8") == 1
    audited = set(A.AUDITED_MORE)
    assert {c for c in inline if "combination" in c[4]} <= audited and {c[0] for c in audited & set(inline)} == set(A.INLINE_KINDS)
    assert {c for c in cols if "combination" in c[4]} <= audited
    assert {(c[0], c[3]) for c in audited if c[2] == "pseudohuber" and c[6] == A.NO_FRACTIONS} == \
        {(k, p) for k in ("sampled", "deep_sampled") for p in ("pairs", "constrained_regularised")}
    # of a tree's features a level keeps fewer, and a node fewer again
    for nfeat, colsample in ((8, 0.5), (4, 1.0)):
        n_sel = P.num_selected(nfeat, colsample)
        n_lvl = K.count(A.COL_FRACTIONS[0], n_sel)
        assert n_sel > n_lvl > K.count(A.COL_FRACTIONS[1], n_lvl) >= 1


@pytest.mark.parametrize("case", EVERY_CASE, ids=A.more_id)
def test_a_case_reaches_its_setting_and_its_restated_trees_pass_the_audit(case):
    want = A.reaches_more(case)
    x, y, w, cuts, _, _ = A.restated_more(case)
    seen = A.profile_more(case)
    constrained = bool(A.POLICIES[case[3]][2])
    audits = A.audits_more(case, x, y, w, cuts, want["all_trees"])
    worst = {"loss_chg": 0.0, "weight": 0.0}
    for r, a in enumerate(audits):
        assert a.violations() == [], (case, r)
        assert a.stats["records"] == a.size + a.size // 2, "a base_weight a node and a loss_chg a split"
        if constrained:
            assert A.sweep_violations(want["all_trees"][r], x, cuts, A.CONSTRAINTS) == 0, (case, r)
        # the restatement's own doubles against the exact values, as a fraction of the derived bounds
        for p in a.order:
            if want["all_trees"][r]["left"][p] >= 0:
                best = seen[r][p]["best"]
                assert best[1:4] == a.split_of(p)
                cand = [c for c in a.candidates(p) if c[1:4] == best[1:4]][0]
                loss, e = a.loss(p, cand)
                worst["loss_chg"] = max(worst["loss_chg"], float(abs(Fraction(float(best[0])) - loss)) / e)
                if constrained:
                    for double, exact, bound in ((best[6], cand[6], cand[7]), (best[7], cand[8], cand[9])):
                        if double != exact[0] / exact[1]:
                            worst["weight"] = max(worst["weight"], float(abs(Fraction(double) - Fraction(*exact))) / bound)
    records, pinned = (sum(a.stats[k] for a in audits) for k in ("records", "pinned"))
    splits, decided = [a.size // 2 for a in audits], [A.decided(a) for a in audits]
    print(A.more_id(case), "pinned %d of %d (%.2f %%)," % (pinned, records, 100.0 * pinned / records), "split nodes", splits, "decided", decided,
          "the restatement's error / bound:", worst)
    assert pinned >= 0.95 * records, "the bounds pin nearly every float32 record to one value"
    assert worst["loss_chg"] < 1 and worst["weight"] < 1, "the reference inside the derived bounds"
    if case in A.AUDITED_MORE:
        assert min(splits) >= 10, "every audited tree has splits to audit"
        assert sum(decided) >= 10, "and the call splits at which a wrong choice would be reported"


# ---- the audit bites what it newly claims to see ----

def copy_of(tree):
    return {k: np.asarray(tree[k]).copy() for k in G.ARRAYS}


def sound_trees(case):
    """-> per restated tree of the case (the tree, what it was grown on, its audit)."""
    x, y, w, cuts, _, want = A.restated_more(case)
    trees = want["all_trees"]
    out = []
    for r in range(len(trees)):
        inputs = A.round_inputs(case[0], case[3], A.case_hyper(case), x, y, w, cuts, trees, r, **A.more_inputs(case))
        a = A.Audit(tree=trees[r], **inputs)
        assert a.violations() == []
        out.append((copy_of(trees[r]), inputs, a))
    return out


def found_in(tree, inputs):
    return A.Audit(tree=tree, **inputs).violations()


def leaves_below(tree, p):
    return tree["left"][p] >= 0 and tree["left"][tree["left"][p]] < 0 and tree["left"][tree["right"][p]] < 0


def resplit(tree, inputs, a, p, f, j, dl):
    """The tree with node p (a split over two leaves) split at (f, j, dl) instead, the records of p and its children as the
    exact values make them: every sum and weight consistent with the new split."""
    cut_ptr, cut_values = inputs["cuts"]
    cand = [c for c in a.candidates(p) if c[1:4] == (f, j, dl)][0]
    GL, HL, wL, wR = cand[4], cand[5], cand[6], cand[8]
    t = copy_of(tree)
    t["feature"][p], t["default_left"][p], t["value"][p] = f, dl, cut_values[int(cut_ptr[f]) + j]
    t["loss_chg"][p] = F32(float(a.loss(p, cand)[0]))
    for c, H, w in ((int(t["left"][p]), HL, wL), (int(t["right"][p]), a.H[p] - HL, wR)):
        t["sum_hess"][c], t["base_weight"][c] = F32(float(H) * 2.0 ** -24), F32(w[0] / w[1])
        t["value"][c] = t["base_weight"][c] * F32(inputs["eta"])
    return t


NODE_SETS = A.COLSAMPLE_CASES[0]        # sampled, pseudo-Huber, the combination, under both fractions


def with_the_trees_list(case, inputs, r):
    """The inputs with the tree's list in place of the node sets."""
    kw = A.case_hyper(case)
    return dict(inputs, kept=P.features(kw["seed"], r, A.nfeat_of(case), kw["colsample_bytree"]))


def test_the_audit_reports_a_split_on_a_column_that_is_not_the_nodes_own():
    """The split of a narrowed node is replaced by the winner over the tree's list, which lies outside S_node(p)."""
    tried = 0
    for r, (tree, inputs, a) in enumerate(sound_trees(NODE_SETS)):
        free = A.Audit(tree=tree, **with_the_trees_list(NODE_SETS, inputs, r))        # the same rows, every column of the tree
        for p in a.order:
            if not leaves_below(tree, p):
                continue
            loss, e, f, j, dl = free.ranked(p)[0]
            if f in a.kept_at(p):
                continue
            found = found_in(resplit(tree, inputs, free, p, f, j, dl), inputs)
            assert [v[:2] for v in found] == [(p, "structure")], (p, found)
            over_the_list = found_in(resplit(tree, inputs, free, p, f, j, dl), with_the_trees_list(NODE_SETS, inputs, r))
            assert not {v[0] for v in over_the_list} & {p, int(tree["left"][p]), int(tree["right"][p])}, "sound but for the set"
            tried += 1
    assert tried >= 3


def test_the_audit_with_the_trees_list_in_place_of_the_node_sets_reports_narrowed_nodes():
    """What the audit asked before it knew the node sets: the best of the tree's columns.  The trees are not that."""
    x, y, w, cuts, _, want = A.restated_more(NODE_SETS)
    for r, (tree, inputs, a) in enumerate(sound_trees(NODE_SETS)):
        narrowed = {e["p"] for e in want["draws"][r] if e["free"] is not None and e["free"] not in e["node"]}
        found = found_in(tree, with_the_trees_list(NODE_SETS, inputs, r))
        assert found and {v[1] for v in found} <= {"optimality", "closure"}, found
        assert {v[0] for v in found} <= narrowed, "only at nodes whose best candidate is not their own"
        assert any(v[1] == "optimality" for v in found), found


def test_the_audit_reports_a_bag_that_is_left_out():
    case = [c for c in A.AUDITED_MORE if c[0] == "sampled" and c[6] == A.NO_FRACTIONS and c[2] == "pseudohuber"][0]
    for tree, inputs, a in sound_trees(case):
        assert not np.all(inputs["in_bag"]), "a bag that leaves rows out"
        found = found_in(tree, dict(inputs, in_bag=None))
        assert (0, "sum_hess") in {v[:2] for v in found}, found
        assert sum(1 for v in found if v[1] == "sum_hess") > a.size // 2, "nearly every node holds rows out of the bag"


GAMMA_CASE = A.INLINE_CASES[0]          # plain, gamma 0.5


def test_the_audit_reports_a_split_below_a_larger_gamma_and_a_leaf_closed_above_a_smaller():
    assert A.case_hyper(GAMMA_CASE)["gamma"] == 0.5
    bit = 0
    for tree, inputs, a in sound_trees(GAMMA_CASE):
        losses = {p: float(tree["loss_chg"][p]) for p in a.order if tree["left"][p] >= 0}
        larger = 2.0 * min(losses.values())
        below = {p for p, v in losses.items() if v < 0.99 * larger}
        assert below and len(below) < len(losses), "a gamma between the splits' loss_chg"
        found = found_in(tree, dict(inputs, gamma=larger))
        assert {v[0] for v in found if v[1] == "gamma"} >= below and {v[1] for v in found} == {"gamma"}, found
        # at gamma 0 a node that gamma closed is closed wrongly where its best candidate gains anything at all
        closed = [p for p in a.order if tree["left"][p] < 0 and a.evaluated(p) and a.candidates(p)]
        wrongly = {p for p in closed if a.ranked(p)[0][0] > a.ranked(p)[0][1]}
        found = found_in(tree, dict(inputs, gamma=0.0))
        assert {v[:2] for v in found} == {(p, "closure") for p in wrongly}, found
        bit += len(wrongly)
    assert bit >= 1, "gamma closes a node whose best candidate lies between 0 and gamma"


def test_the_audit_reports_a_child_of_fewer_rows_than_min_child_rows():
    """A tree of the plain call grown at min_child_rows = 3 holds a child of exactly three rows: audited at 4, the split above
    it is not admitted (and the child, a leaf above max_depth with six rows or more, is another matter: closure is not asked
    of it here)."""
    case = [c for c in A.INLINE_CASES if c[0] == "plain" and c[4] == "combination"][0]
    assert A.case_hyper(case)["min_child_rows"] == 3
    bit = 0
    for tree, inputs, a in sound_trees(case):
        small = {int(tree["parent"][c]) & 0x7FFFFFFF for c in a.order[1:] if a.H[c] == 3 * A.ONE}
        found = found_in(tree, dict(inputs, mcw=4.0))
        assert {v[0] for v in found if v[1] == "admission"} >= small, found
        assert all(v[1] in ("admission", "optimality", "closure") for v in found), found
        bit += len(small)
    assert bit >= 1, "a child of exactly three rows"


def test_the_audit_reports_a_decided_split_swapped_for_its_runner_up():
    tried = 0
    for case in (A.INLINE_CASES[8], NODE_SETS):        # the plain call at its combination, and the node sets
        for tree, inputs, a in sound_trees(case):
            for p in a.order:
                if not leaves_below(tree, p):
                    continue
                ranked = a.ranked(p)
                if len(ranked) < 2 or tuple(ranked[0][2:]) != a.split_of(p) or not ranked[0][0] - ranked[1][0] > ranked[0][1] + ranked[1][1]:
                    continue                       # (a tie within the bounds is not judged)
                found = found_in(resplit(tree, inputs, a, p, *ranked[1][2:]), inputs)
                assert [v[:2] for v in found] == [(p, "optimality")], (p, found)
                tried += 1
    assert tried >= 6


def test_a_callable_that_takes_nothing_away_gives_the_verdicts_of_the_list():
    kind, _, policy, setting, seed = A.AUDITED[0]
    x, y, w, cuts, _, want = A.restated(kind, policy, setting, seed)
    trees = want["all_trees"]
    for r, t in enumerate(trees):
        inputs = A.round_inputs(kind, policy, setting, x, y, w, cuts, trees, r)
        assert isinstance(inputs["kept"], list)
        sets = A.node_sets(0, r, inputs["kept"], 1.0, 1.0)
        # sound, and with a planted error each
        moved = copy_of(t)
        p = [p for p in range(len(t["left"])) if t["left"][p] >= 0][1]
        moved["feature"][p] = (int(moved["feature"][p]) + 1) % A.NFEAT
        off = copy_of(t)
        off["loss_chg"][0] = -off["loss_chg"][0]
        for tree in (t, moved, off):
            by_list, by_sets = A.Audit(tree=tree, **inputs), A.Audit(tree=tree, **dict(inputs, kept=sets))
            assert by_sets.violations() == by_list.violations() and by_sets.stats == by_list.stats
            assert (tree is t) == (by_list.violations() == [])
            assert A.decided(by_sets) == A.decided(by_list)
