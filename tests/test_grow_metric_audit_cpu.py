"""The metric audit (tests/grow_metric_audit_support.py) over the restatements' trees and arrays, without a GPU: in this
file the restatement is the thing under audit.  The cases are the GPU tables' (tests/test_gpu_grow_metric_audit.py), and
what is shared with that file lives here: the inputs, the restated trees of a kind, the restated arrays of a case, and the
conditions a case has to meet so that the audit can see a fault (docs/34_metric_audit_tests.md).

A restated case grows its trees once per kind (the metric moves no tree at patience 0) and computes each metric's arrays
from the restatement's own pieces: its held-out walk, its residuals, its sums and its values."""
import functools
import math

import numpy as np
import pytest

from tests import grow_eval_support as E
from tests import grow_metric_audit_support as M
from tests import grow_objective_support as O
from tests import grow_quantile_support as Q
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests import grow_weighted_support as W

F32 = np.float32
NAN = float("nan")
BELOW_256 = np.nextafter(F32(256.0), F32(0.0))


# ---- shared with the GPU tests ----

def off_grid_weights(rng, n, keep=()):
    """float32 weights whose 2^24-fold is no whole number for most: draws below 0.5 (a float32 below 0.5 has bits under 2^-24),
    draws in [0.5, 2), ties (k + 1/2) * 2^-24 for odd and even k, and zeros.  The rows `keep` hold a weight that is none of
    those zeros.  No weight lies below 2^-6, which keeps the bound of the audit four orders under the value."""
    w = np.where(rng.random(n) < 0.6, rng.uniform(2.0 ** -6, 0.5, n), rng.uniform(0.5, 2.0, n)).astype(F32)
    ties = rng.random(n) < 0.08
    k = rng.integers(1 << 20, 1 << 23, n)
    w[ties] = ((2 * k + 1).astype(np.float64) * 2.0 ** -25).astype(F32)[ties]
    w[rng.random(n) < 0.05] = 0.0
    for r in keep:
        w[r] = F32(0.3000001)
    return w


def special_rows(n, trips=()):
    """The rows whose loss the conditions ask a case to notice: the last, the last of the last full wave, the first past each trip."""
    return sorted({n - 1, n // 64 * 64 - 1} | {t for t in trips if t < n})


@functools.lru_cache(maxsize=None)
def inputs(seed=3401, n=M.N, held_out=M.HELD, bins=64, trips=(), etrips=()):
    """grow_objective_support.inputs, changed as docs/34 says -> (x, y, w, cuts, ev); not to be changed by a caller."""
    x, y, _, cuts, ev = O.inputs(n, seed, M.NFEAT, bins, held_out)
    if n > 100000:
        cuts = G.quantile_cuts(x[:M.N], NAN, bins)
    rng = np.random.default_rng(seed + 1)
    w = off_grid_weights(rng, n, special_rows(n, trips))
    ex, _, ey, _ = ev
    ex = np.where(np.isnan(ex[:, :M.NFEAT - 1]), F32(M.MISSING), ex[:, :M.NFEAT - 1]).astype(F32)      # one column fewer, its own missing
    ptr, vals = cuts
    for i in range(64):                                # rows on a cut in every column, or one float to either side of it
        for c in range(ex.shape[1]):
            cut = F32(vals[int(ptr[c]) + int(rng.integers(0, int(ptr[c + 1] - ptr[c])))])
            ex[5 + 19 * i, c] = (cut, np.nextafter(cut, F32(-np.inf)), np.nextafter(cut, F32(np.inf)))[(i + c) % 3]
    ew = off_grid_weights(rng, held_out, special_rows(held_out, etrips))
    return x, y, w, cuts, (np.ascontiguousarray(ex), M.MISSING, ey, ew)


def kind_hyper(kind, rounds=M.ROUNDS, deep_depth=11, max_depth=None):
    kw = dict(O.kind_kw("weighted" if kind == "eval" else kind, deep_depth), rounds=rounds)
    if max_depth is not None:
        kw["max_depth"] = max_depth
    if kind == "eval":
        del kw["min_child_weight"]
        kw["min_child_rows"] = 1
    return kw


@functools.lru_cache(maxsize=None)
def restated_trees(kind, rounds=M.ROUNDS, max_depth=None, seed=3401):
    """The restated trees of a kind under squared error, and the restatement's margins of both sets after every round."""
    x, y, w, cuts, ev = inputs(seed)
    kw = kind_hyper(kind, rounds, max_depth=max_depth)
    start, estart = np.full(len(y), O.BASE, F32), np.full(len(ev[2]), O.BASE, F32)
    if kind == "eval":
        out = G.boost(start, x, NAN, y, cuts, M.NFEAT, rounds=rounds, max_depth=kw["max_depth"], eta=kw["eta"], lam=kw["reg_lambda"],
                      min_child_rows=1)
        trees, preds = out["trees"], [start] + out["preds"]
    else:
        out = O.boost("squarederror", 1.0, start, x, NAN, y, w, cuts, M.NFEAT, rounds=rounds, max_depth=kw["max_depth"], eta=kw["eta"],
                      lam=kw["reg_lambda"], min_child_weight=kw["min_child_weight"], subsample=kw.get("subsample", 1.0),
                      colsample_bytree=kw.get("colsample_bytree", 1.0), seed=kw.get("seed", 0))
        trees, preds = out["all_trees"], out["preds"]
    epreds = [estart]
    for t in trees:
        nxt = epreds[-1] + E.walk(t, ev[0], ev[1])
        assert nxt.dtype == F32
        epreds.append(nxt)
    return trees, preds, epreds


def docs_of(trees):
    return [G.tree_doc(t, i, M.NFEAT) for i, t in enumerate(trees)]


def mirrored(ev):
    """The held-out set with its labels mirrored at the base margin: whatever the trees learn makes its error worse."""
    return ev[0], ev[1], (F32(2.0 * O.BASE) - ev[2]).astype(F32), ev[3]


def restated_got(kind, metric, slope, alpha, rounds=M.ROUNDS, patience=0, max_depth=None, seed=3401, mirror=False):
    """What the restatement says the call returns -> (the dict of a boost call, its exact held-out sums)."""
    x, y, w, cuts, ev = inputs(seed)
    if mirror:
        ev = mirrored(ev)
    trees, preds, epreds = restated_trees(kind, rounds, max_depth, seed)
    if kind == "eval":
        sums = [[E.sum_squares(p, yy) for p in ps] for ps, yy in ((preds, y), (epreds, ev[2]))]
        vals = [[E.rmse(s, len(yy)) for s in ss] for ss, yy in zip(sums, (y, ev[2]))]
    else:
        sets = ((preds, y, W.hess_fixed(w)), (epreds, ev[2], W.hess_fixed(ev[3])))
        sums = [[Q.metric_sum(metric, slope, alpha, W.residuals(p, yy), hq) for p in ps] for ps, yy, hq in sets]
        vals = [[Q.metric_value(metric, s, int(hq.astype(object).sum())) for s in ss] for ss, (_, _, hq) in zip(sums, sets)]
    run, best = E.stop_rule(lambda t: sums[1][t], rounds, patience)
    return {"train_rmse": np.asarray(vals[0][:run + 1]), "eval_rmse": np.asarray(vals[1][:run + 1]), "rounds_run": run, "best_round": best}, sums[1]


def sets_of(kind, x, y, w, ev, start=None, estart=None):
    """The two sets as the audit takes them: rows, missing, labels, weights (None for the Eval call), starting margins."""
    start = np.full(len(y), O.BASE, F32) if start is None else start
    estart = np.full(len(ev[2]), O.BASE, F32) if estart is None else estart
    counted = kind == "eval"
    return (x, NAN, y, None if counted else w, start), (ev[0], ev[1], ev[2], None if counted else ev[3], estart)


def audit_of(case, trees, x, y, w, ev, truth=True, **more):
    kind, metric, slope, alpha, _ = case
    train, held = sets_of(kind, x, y, w, ev)
    return M.MetricAudit(metric, trees, train, held, slope=slope, alpha=alpha, counted=kind == "eval", truth=truth, **more)


def conditions(audit, trips=(), etrips=(), need_cut_rows=True):
    """What a case has to meet for the audit to see a fault (docs/34): every such change moves the defined double."""
    for name, tr in (("train", trips), ("eval", etrips)):
        x, missing, y, w, start = audit.sets[name]
        T = len(audit.defined[name]) - 1
        assert len(set(audit.defined[name])) >= 2, (name, "two distinct values in the array")
        for r in special_rows(len(y), tr):
            for t in range(T + 1):
                assert audit.without_row(name, t, r) != audit.defined[name][t], (name, "row", r, "round", t)
        # one missing value sent against its default: the first row that tree 1 then leaves elsewhere
        flipped = start + M.leaf_values(audit.trees[0], x, missing, flip_default=True)
        assert flipped.dtype == F32
        moved = np.flatnonzero((flipped != audit.preds[name][1]) & (M.weights_fixed(w, len(y)) > 0))
        assert len(moved) > 0, (name, "a missing value on a split")
        r = int(moved[0])
        assert audit.without_row(name, 1, r, pred=flipped[r]) != audit.defined[name][1], (name, "a default", r)
    if audit.true["train"]:
        for name in audit.sets:
            for t, (b, v) in enumerate(zip(audit.bounds[name], audit.true[name])):
                assert b <= v * M.D("1e-4"), (name, t, float(b), float(v))
    if need_cut_rows:                                  # a held-out row on a split it reaches: x <= c would lead it elsewhere
        x, missing, y, w, start = audit.sets["eval"]
        other = M.margins(audit.trees, x, missing, start, less=np.less_equal)[-1]
        assert np.any((other != audit.preds["eval"][-1]) & (audit.hq("eval") > 0)), "no held-out row sits on a split of the trees"


def worst_ratio(audit, got):
    return max(audit.ratio(name, t, v) for name, key in (("train", "train_rmse"), ("eval", "eval_rmse")) for t, v in enumerate(got[key]))


@functools.lru_cache(maxsize=None)
def restated_audit(case):
    kind, metric, slope, alpha, _ = case
    x, y, w, cuts, ev = inputs()
    trees, _, _ = restated_trees(kind)
    return audit_of(case, docs_of(trees), x, y, w, ev)


# ---- 1. no violation on any case of the GPU tables, and the bound holds ----

@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_no_violation_on_the_restated_case_and_the_bound_holds(case):
    kind, metric, slope, alpha, _ = case
    got, _ = restated_got(kind, metric, slope, alpha)
    audit = restated_audit(case)
    assert audit.violations(got, M.ROUNDS) == []
    conditions(audit)
    ratio = worst_ratio(audit, got)
    rel = max(float(b / v) for name in audit.sets for b, v in zip(audit.bounds[name], audit.true[name]))
    print(f"{M.case_id(case)}: worst |restated - true| / bound = {ratio:.4f}; worst bound / true = {rel:.2e}")
    assert ratio <= 1.0, ratio


def test_the_inputs_are_what_the_cases_need():
    x, y, w, cuts, ev = inputs()
    for ww in (w, ev[3]):
        scaled = ww.astype(np.float64) * 2.0 ** 24
        frac = scaled - np.floor(scaled)
        k = np.floor(scaled[frac == 0.5]).astype(np.int64)
        assert np.count_nonzero(frac != 0) > len(ww) // 4 and np.count_nonzero((frac != 0) & (frac != 0.5)) > 100, "weights off the 2^-24 grid"
        assert np.count_nonzero(k % 2 == 0) > 10 and np.count_nonzero(k % 2 == 1) > 10, "ties above odd and even k"
        assert np.count_nonzero(ww == 0) > 10 and ww[ww > 0].min() >= 2.0 ** -6
    assert ev[0].shape == (M.HELD, M.NFEAT - 1) and ev[1] == M.MISSING and np.count_nonzero(ev[0] == F32(M.MISSING)) > 100
    assert not np.isnan(ev[0]).any()


@pytest.mark.parametrize("case", M.STOP_CASES, ids=M.case_id)
def test_the_stop_rule_on_the_restated_curve(case):
    kind, metric, slope, alpha, patience = case
    depth = 3 if kind == "weighted" else 10
    got, esums = restated_got(kind, metric, slope, alpha, rounds=12, patience=patience, max_depth=depth)
    x, y, w, cuts, ev = inputs()
    trees, _, _ = restated_trees(kind, 12, depth)
    audit = audit_of((kind, metric, slope, alpha, None), docs_of(trees[:got["rounds_run"]]), x, y, w, ev, truth=False)
    assert audit.violations(got, 12, patience) == []
    assert audit.sums["eval"] == esums[:got["rounds_run"] + 1]


def test_a_held_out_set_that_only_gets_worse_stops_at_best_round_0():
    x, y, w, cuts, ev = inputs()
    got, esums = restated_got("weighted", "mae", 1.0, 0.5, rounds=12, patience=2, max_depth=3, mirror=True)
    assert (got["rounds_run"], got["best_round"]) == (2, 0) and esums[0] < esums[1] < esums[2]
    trees, _, _ = restated_trees("weighted", 12, 3)
    audit = audit_of(("weighted", "mae", 1.0, 0.5, None), docs_of(trees[:2]), x, y, w, mirrored(ev), truth=False)
    assert audit.violations(got, 12, 2) == []


def test_the_stop_cases_reach_what_they_are_meant_to():
    stops = {c: restated_got(c[0], c[1], c[2], c[3], rounds=12, patience=c[4], max_depth=3 if c[0] == "weighted" else 10)[0] for c in M.STOP_CASES}
    inside = [c for c, g in stops.items() if 0 < g["best_round"] < g["rounds_run"] < 12]
    assert inside, {M.case_id(c): (g["rounds_run"], g["best_round"]) for c, g in stops.items()}


# ---- 2. it bites ----

BITE = ("weighted", "mae", 1.0, 0.5, "host")


def planted_got(case, drop=None, hq_of=None, f64=False, value=None, metric=None, bag=False, **walk):
    """The arrays of a call that is wrong in one way, over the restated trees of the case."""
    kind, _metric, slope, alpha, _ = case
    metric = metric or _metric
    x, y, w, cuts, ev = inputs()
    trees = docs_of(restated_trees(kind)[0])
    out = {}
    for key, (xx, missing, yy, ww, start), planted in zip(("train_rmse", "eval_rmse"), sets_of(kind, x, y, w, ev), ({}, walk)):
        if f64:
            acc, preds = start.astype(np.float64), [start]
            for t in trees:
                acc = acc + M.leaf_values(t, xx, missing).astype(np.float64)
                preds.append(acc.astype(F32))
        else:
            preds = M.margins(trees, xx, missing, start, **planted)
        hq = (hq_of or M.weights_fixed)(ww, len(yy))
        vals = []
        for t, p in enumerate(preds):
            h = hq.copy()
            if drop is not None and drop < len(h):
                h[drop] = 0
            if bag and t >= 1 and key == "train_rmse":
                h = np.where(P.bag(11, t - 1, len(yy), 0.5), h, 0)
            S = M.exact_sum(h, M.terms(metric, M.residual(p, yy), slope, alpha))
            v = M.defined(metric, S, M.exact_sum(h))
            vals.append(value(v) if value else v)
        out[key] = np.asarray(vals)
    out["rounds_run"], out["best_round"] = M.ROUNDS, restated_got(kind, metric, slope, alpha)[0]["best_round"]
    return out


def reported(case, got, **more):
    audit = restated_audit(case) if not more else audit_of(case, docs_of(restated_trees(case[0])[0]), *inputs()[:3], inputs()[4], **more)
    v = audit.violations(got, M.ROUNDS)
    return {c for c, *_ in v}, {s for _, s, *_ in v}, v


def truncated(w, n):
    return np.floor(np.asarray(w, F32).astype(np.float64) * 2.0 ** 24).astype(np.int64)


def test_a_held_out_row_walked_by_less_or_equal_is_reported():
    checks, sets, v = reported(BITE, planted_got(BITE, less=np.less_equal))
    assert checks == {"defined", "truth"} and sets == {"eval"}, v
    x, y, w, cuts, ev = inputs()
    ex = ev[0].copy()
    ex[5:5 + 19 * 64:19] += F32(0.001)                   # the rows moved off their cuts: nothing to report
    audit = audit_of(BITE, docs_of(restated_trees("weighted")[0]), x, y, w, (ex, ev[1], ev[2], ev[3]), truth=False)
    other = audit_of(BITE, docs_of(restated_trees("weighted")[0]), x, y, w, (ex, ev[1], ev[2], ev[3]), truth=False, less=np.less_equal)
    assert audit.defined["eval"] == other.defined["eval"], "reported only because rows sit exactly on cuts"


def test_missing_always_sent_left_is_reported():
    checks, sets, v = reported(BITE, planted_got(BITE, missing_left=True))
    assert checks == {"defined", "truth"} and sets == {"eval"}, v


def test_a_margin_summed_in_float64_is_reported():
    checks, sets, v = reported(BITE, planted_got(BITE, f64=True))
    assert checks == {"defined"} and all(t >= 2 for _, _, t, *_ in v), v


def test_one_row_left_out_is_reported():
    checks, sets, v = reported(BITE, planted_got(BITE, drop=M.N // 64 * 64 - 1))
    assert "defined" in checks and sets == {"train"}, v       # the held-out set is shorter: its row 4031 does not exist
    checks, sets, v = reported(BITE, planted_got(BITE, drop=M.HELD - 1))
    assert "defined" in checks and sets == {"train", "eval"}, v


def test_the_bag_applied_to_the_metric_is_reported():
    case = ("sampled", "mae", 1.0, 0.5, "host")
    checks, sets, v = reported(case, planted_got(case, bag=True))
    assert checks == {"defined", "truth"} and sets == {"train"} and all(t >= 1 for _, _, t, *_ in v), v


def test_a_truncated_weight_is_reported():
    checks, sets, v = reported(BITE, planted_got(BITE, hq_of=truncated))
    assert checks == {"defined"} and sets == {"train", "eval"}, v


def test_mae_reported_for_pseudohuber_is_reported():
    case = ("weighted", "pseudohuber", 3.7, 0.5, "host")
    got = planted_got(case, metric="mae")
    checks, sets, v = reported(case, got)
    assert checks >= {"defined", "truth"}, v                     # and "stop" where the two curves turn at different rounds
    checks, sets, v = reported(case, got, sq_metric="mae")      # the defined value fed the wrong sq: the true value alone objects
    assert checks == {"truth"} and len(v) == 2 * (M.ROUNDS + 1), v


def test_an_rmse_without_its_root_is_reported():
    case = ("weighted", "rmse", 1.0, 0.5, "host")
    checks, sets, v = reported(case, planted_got(case, value=lambda r: r * r))
    assert checks == {"defined", "truth"} and len(v) == 4 * (M.ROUNDS + 1), v


def test_an_unweighted_mean_is_reported():
    checks, sets, v = reported(BITE, planted_got(BITE, hq_of=lambda w, n: np.full(n, M.ONE, np.int64)))
    assert checks == {"defined", "truth"} and sets == {"train", "eval"}, v


def test_a_tie_taken_as_an_improvement_is_reported():
    x, y, w, cuts, ev, want = Q.tie_case()
    assert want["eval_sums"][1] == want["eval_sums"][0] and (want["rounds_run"], want["best_round"]) == (1, 0)
    train = (x, NAN, y, w, np.full(len(y), Q.BASE, F32))
    held = (ev[0], ev[1], ev[2], ev[3], np.full(len(ev[2]), Q.BASE, F32))
    trees = [G.tree_doc(t, i, 3) for i, t in enumerate(want["all_trees"])]
    got = dict(train_rmse=np.asarray(want["train_rmse"]), eval_rmse=np.asarray(want["eval_rmse"]), rounds_run=1, best_round=0)
    audit = M.MetricAudit("quantile", trees[:1], train, held, alpha=0.5, truth=False)
    assert audit.violations(got, 3, 1) == []
    # the rule with <=: every round ties, so it never stops and best moves to the last round
    every = M.MetricAudit("quantile", [trees[0]] * 3, train, held, alpha=0.5, truth=False)
    lenient = dict(train_rmse=np.asarray(every.defined["train"]), eval_rmse=np.asarray(every.defined["eval"]), rounds_run=3, best_round=3)
    v = every.violations(lenient, 3, 1)
    assert [c for c, *_ in v] == ["stop"] and v[0][3:] == ((3, 3), (1, 0)), v


def test_best_of_the_doubles_is_reported_where_two_sums_share_a_double():
    S = [(1 << 80) + 2, (1 << 80) + 1, (1 << 80) + 3]
    W = 1 << 30
    audit = M.MetricAudit.from_sums("mae", [5 << 60, 4 << 60, 3 << 60], W, S, W)
    assert audit.defined["eval"][0] == audit.defined["eval"][1] and float(S[0]) == float(S[1])
    assert M.stop_rule(S, 2, 1) == (2, 1)
    by_doubles = M.stop_rule([float(s) for s in S], 2, 1)
    assert by_doubles == (1, 0)
    right = dict(train_rmse=audit.defined["train"], eval_rmse=audit.defined["eval"], rounds_run=2, best_round=1)
    assert audit.violations(right, 2, 1) == []
    wrong = dict(train_rmse=audit.defined["train"][:2], eval_rmse=audit.defined["eval"][:2], rounds_run=1, best_round=0)
    v = audit.violations(wrong, 2, 1)
    assert [c for c, *_ in v] == ["stop"], v


# ---- 3. the audit's own pieces ----

def test_the_walk_takes_the_default_for_nan_missing_and_a_lacking_column():
    tree = {"left_children": [1, -1, 3, -1, -1], "right_children": [2, -1, 4, -1, -1], "split_indices": [0, 0, 2, 0, 0],
            "default_left": [1, 0, 0, 0, 0], "split_conditions": [0.5, 1.0, 0.25, 2.0, 3.0]}
    x = np.asarray([[0.25, 0.0], [0.5, 0.0], [NAN, 0.0], [-999.0, 0.0], [0.75, NAN], [np.nextafter(F32(0.5), F32(0)), 0.0]], F32)
    assert M.leaf_values(tree, x, -999.0).tolist() == [1.0, 3.0, 1.0, 1.0, 3.0, 1.0]      # feature 2 is lacking: default right
    assert M.leaf_values(tree, x, NAN).tolist() == [1.0, 3.0, 1.0, 1.0, 3.0, 1.0]          # -999 < 0.5 goes left anyway
    assert M.leaf_values(tree, x, -999.0, less=np.less_equal).tolist() == [1.0, 1.0, 1.0, 1.0, 3.0, 1.0]
    assert M.leaf_values(tree, x, -999.0, flip_default=True).tolist() == [1.0, 2.0, 2.0, 2.0, 2.0, 1.0]


def test_the_fixed_point_rounds_ties_to_even_and_the_defined_value_is_the_headers():
    assert M.fixed(np.asarray([1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, -1.5 * 2.0 ** -24, BELOW_256], F32)).tolist() == [2, 2, -2, (1 << 32) - 256]
    assert M.alpha_fixed(0.05) == int(np.rint(np.float64(F32(0.05)) * 2.0 ** 24))
    z = np.asarray([-2.0, 1.0], F32)
    assert M.terms("quantile", z, alpha=0.25).tolist() == [(2 << 24) * (1 << 22), (1 << 24) * (3 << 22)]
    assert M.terms("pseudohuber", np.asarray([0.0, 2.0 ** -70], F32), slope=1.0).tolist() == [0, 0]
    S, Wq = (3 << 72) + 12345, 3 << 24
    assert M.defined("rmse", S, Wq) == math.sqrt((float(S) * 2.0 ** -72) / 3.0)
    assert M.defined("rmse", 48 << 48, 0, counted=True, n=3) == 4.0
    assert M.defined("mae", 6 << 48, Wq) == 2.0 and M.defined("quantile", 6 << 72, Wq) == 2.0
    assert float(M.true_value("pseudohuber", [3.0], [0.0], [1.0], slope=4.0)) == 16.0 * (1.25 - 1.0)
    assert float(M.true_value("quantile", [0.0, 0.0], [1.0, -1.0], None, alpha=0.25)) == 0.5
    assert float(M.true_value("rmse", [0.0, 0.0], [3.0, -4.0], [1.0, 1.0])) == math.sqrt(12.5)
