"""The metric arrays and the stop rule of every boost call against the audit of tests/grow_metric_audit_support.py, on the
GPU: a case is called once, its new trees are read back from XGBoosterSaveModel's JSON, the caller's float rows are walked
through them on the host, and train_rmse[], eval_rmse[], rounds_run and best_round must be what the header defines from the
exact sums over those margins - bit for bit - and lie within the derived bound of the textbook loss in 100 digits.  The
trees are never the restatement's.  Where a call stops early its later trees are gone: a twin booster with patience 0 and
rounds = rounds_run grows them again (the header makes tree t the same tree), its arrays must be the stopped call's, and
its trees are audited.

The inputs, the conditions a case has to meet and the restatements they are asserted from: tests/test_grow_metric_audit_cpu.py.
The kernels: grow_sse_kernel, grow_walk_sse_kernel, their weighted, metric<mae|pseudohuber> and quantile forms, and the
four instances of the deep walk (docs/34_metric_audit_tests.md)."""
import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_metric_audit_support as M
from tests import grow_objective_support as O
from tests import grow_support as G
from tests import test_grow_metric_audit_cpu as T
from tests import visits_support as V
from tests.test_gpu_grow import held
from tests.test_gpu_grow_objective import NAN, ROWS_PAST_A_STRIDE, booster, call, done

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def metric_params(metric, slope, alpha):
    return (("ohx_eval_metric", metric), ("ohx_huber_slope", repr(float(slope))), ("ohx_quantile_alpha", repr(float(alpha))))


def call_eval(torch, b, x, y, cuts, ev, device, **kw):
    """The Eval call, which takes no weights, with the held-out matrix's own missing in either form."""
    if device:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            tx, ty = torch.from_numpy(x).to("cuda"), torch.from_numpy(y).to("cuda")
            tex, tey = torch.from_numpy(ev[0]).to("cuda"), torch.from_numpy(ev[2]).to("cuda")
        s.synchronize()
        d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=x.shape[0], ncol=x.shape[1], missing=NAN)
        ed = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=ev[0].shape[0], ncol=ev[0].shape[1], missing=ev[1])
        got = b.boost_trees_eval_device(d, ty.data_ptr(), len(y), cuts, eval_set=(ed, tey.data_ptr(), len(ev[2])), stream=s.cuda_stream, **kw)
    else:
        d, ed = capi.DMatrix(x, missing=NAN), capi.DMatrix(ev[0], missing=ev[1])
        got = b.boost_trees_eval(d, y, cuts, eval_set=(ed, ev[2]), **kw)
    return got, [d, ed]


def grown(torch, tmp_path, kind, params, x, y, w, cuts, ev, device, b=None, base=O.BASE, **kw):
    """One call -> (the result, the new trees as the saved JSON holds them).  With `b` the call extends that booster, which
    stays open."""
    own = b is None
    b = booster(params, nfeat=M.NFEAT, base=base) if own else b
    before = len(V.doc_trees(held(b, tmp_path)[1]))
    if kind == "eval":
        got, mats = call_eval(torch, b, x, y, cuts, ev, device, **kw)
    else:
        got, mats = call(torch, b, kind, x, y, w, cuts, ev, device=device, **kw)
    trees = V.doc_trees(held(b, tmp_path)[1])[before:]
    done(b, mats) if own else [m.free() for m in mats]
    return got, trees


def same_upto(got, twin, run):
    for k in ("train_rmse", "eval_rmse"):
        assert got[k].tolist() == twin[k].tolist()[:run + 1] and len(got[k]) == run + 1, k


def audited(torch, tmp_path, case, x, y, w, cuts, ev, device, patience=0, truth=True, base=O.BASE, **kw):
    """The call of `case`, and its twin where it stopped early -> (the result, the audit over the library's own trees)."""
    kind, metric, slope, alpha, _ = case
    params = metric_params(metric, slope, alpha) if kind != "eval" else ()
    got, trees = grown(torch, tmp_path, kind, params, x, y, w, cuts, ev, device, base=base, patience=patience, **kw)
    run = got["rounds_run"]
    assert len(trees) == (got["best_round"] if patience >= 1 else kw["rounds"]), "the forest's length"
    if patience >= 1 and run > len(trees):
        if run > 0:
            twin, trees = grown(torch, tmp_path, kind, params, x, y, w, cuts, ev, device, base=base, patience=0, **dict(kw, rounds=run))
            same_upto(got, twin, run)
        assert len(trees) == run
    train, held_set = T.sets_of(kind, x, y, w, ev, np.full(len(y), base, F32), np.full(len(ev[2]), base, F32))
    audit = M.MetricAudit(metric, trees, train, held_set, slope=slope, alpha=alpha, counted=kind == "eval", truth=truth)
    return got, audit


# ---- 1. every kind under every metric ----

@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_every_kind_and_metric_against_the_audit(torch_cuda, tmp_path, case):
    kind, metric, slope, alpha, form = case
    x, y, w, cuts, ev = T.inputs()
    want, _ = T.restated_got(kind, metric, slope, alpha)
    T.conditions(T.restated_audit(case))                       # from the restatement, before the GPU is asked
    got, audit = audited(torch_cuda, tmp_path, case, x, y, w, cuts, ev, form == "device", **T.kind_hyper(kind))
    assert audit.violations(got, M.ROUNDS) == [], M.case_id(case)
    T.conditions(audit)                                        # and of the library's own trees
    print(f"{M.case_id(case)}: worst |returned - true| / bound = {T.worst_ratio(audit, got):.4f}")
    assert got["train_rmse"].tolist() == want["train_rmse"].tolist() and got["eval_rmse"].tolist() == want["eval_rmse"].tolist()


# ---- 2. the deep walks past one trip of their row loop, in both sets ----

def long_n(torch):
    """(n, the rows of one trip of the walk's grid): n past a trip of the device's own grid, and no whole number of waves."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = synth.grow_eval_plan(1 << 30, cus)
    trip = plan["blocks"] * plan["block_rows"]
    assert trip == synth.grow_plan(1 << 30, M.NFEAT, 0, 6, cus)["row_blocks"] * plan["block_rows"], "the streaming grids share a trip"
    n = ROWS_PAST_A_STRIDE if ROWS_PAST_A_STRIDE > trip else trip + 4097 + 64 + 1
    assert n % 64 != 0 and n > trip and synth.grow_eval_plan(n, cus)["blocks"] == plan["blocks"]
    return n, trip


def levels_of(tree):
    """The number of levels below the root that a saved tree reaches."""
    level, depth = [0], 0
    while True:
        level = [c for n in level if tree["left_children"][n] >= 0 for c in (tree["left_children"][n], tree["right_children"][n])]
        if not level:
            return depth
        depth += 1


LONG = (("deep", "rmse", 1.0, 0.5, "host"), ("deep", "mae", 1.0, 0.5, "device"), ("deep", "pseudohuber", 3.7, 0.5, "host"),
        ("deep", "quantile", 1.0, 0.05, "device"), ("deep_sampled", "mae", 1.0, 0.5, "host"))


@pytest.mark.parametrize("case", LONG, ids=M.case_id)
def test_the_deep_walks_past_one_trip_in_both_sets(torch_cuda, tmp_path, case):
    """n training rows and n held-out rows at depth 10, two rounds.  The host side is the vectorised walk of the library's
    trees and the integer sums; nothing is restated and the second reference is left out."""
    n, trip = long_n(torch_cuda)
    x, y, w, cuts, ev = T.inputs(3402, n, n, 16, (trip,), (trip,))
    assert len(y) == len(ev[2]) == n and w[trip] > 0 and ev[3][trip] > 0
    kw = T.kind_hyper(case[0], rounds=2, deep_depth=10)
    got, audit = audited(torch_cuda, tmp_path, case, x, y, w, cuts, ev, case[4] == "device", truth=False, **kw)
    assert audit.violations(got, 2) == [], M.case_id(case)
    assert kw["max_depth"] == 10 and all(levels_of(t) > 8 for t in audit.trees), "max_depth past 8 takes the walk over the node table in HBM"
    T.conditions(audit, (trip,), (trip,))


# ---- 3. large terms ----

def large_inputs():
    """4097 rows a set, a booster whose base margin is 0, and one cut: feature 0 at 0.  The training labels sit half a unit to
    either side of 0 by the sign of x0, so every tree is the stump x0 < 0 and its leaves pull every held-out residual inward;
    every held-out residual starts one float32 step inside 256, of both signs, and every weight is one step under 256."""
    rng = np.random.default_rng(3403)
    n = 4097
    x = rng.standard_normal((n, M.NFEAT)).astype(F32)
    ex = rng.standard_normal((n, M.NFEAT - 1)).astype(F32)
    y = np.where(x[:, 0] < 0, F32(-0.5), F32(0.5)).astype(F32)
    ey = np.where(ex[:, 0] < 0, -T.BELOW_256, T.BELOW_256).astype(F32)
    w = np.full(n, T.BELOW_256, F32)
    cuts = (np.asarray([0, 1, 1, 1, 1], np.uint64), np.asarray([0.0], F32))
    return x, y, w, cuts, (ex, M.MISSING, ey, w.copy())


@pytest.mark.parametrize("case", tuple(("weighted",) + s + ("host",) for s in M.SETTINGS[:3] + M.SETTINGS[5:]), ids=M.case_id)
def test_large_terms_under_every_metric(torch_cuda, tmp_path, case):
    x, y, w, cuts, ev = large_inputs()
    kw = dict(O.kind_kw("weighted"), rounds=2, max_depth=1)
    got, audit = audited(torch_cuda, tmp_path, case, x, y, w, cuts, ev, False, base=0.0, **kw)
    assert [t["split_conditions"][0] for t in audit.trees] == [0.0, 0.0] and all(len(t["left_children"]) == 3 for t in audit.trees)
    z0 = M.residual(audit.preds["eval"][0], ev[2])
    assert np.all(np.abs(z0) == T.BELOW_256) and (z0 > 0).any() and (z0 < 0).any()
    assert all(s > 1 << 64 for s in audit.sums["eval"]), "three words of the sum are in use"
    assert audit.violations(got, 2) == [], M.case_id(case)
    assert len(set(got["eval_rmse"].tolist())) == 3 and len(set(got["train_rmse"].tolist())) == 3


# ---- 4. a forest that has trees ----

def test_a_second_call_on_a_forest_that_has_trees(torch_cuda, tmp_path):
    """One handle: the Sampled call under mae at depth 6, then under quantile at depth 3.  The second call's starting margins
    are XGBoosterPredict(option_mask = 1) of the booster as it stood."""
    x, y, w, cuts, ev = T.inputs()
    b = booster(metric_params("mae", 1.0, 0.5), nfeat=M.NFEAT)
    kw = T.kind_hyper("sampled", rounds=2)
    got1, trees1 = grown(torch_cuda, tmp_path, "sampled", (), x, y, w, cuts, ev, False, b=b, **kw)
    first = M.MetricAudit("mae", trees1, *T.sets_of("sampled", x, y, w, ev))
    assert first.violations(got1, 2) == []
    d, ed = capi.DMatrix(x, missing=NAN), capi.DMatrix(ev[0], missing=ev[1])
    start, estart = b.predict(d, option_mask=1).astype(F32), b.predict(ed, option_mask=1).astype(F32)
    assert np.array_equal(start, first.preds["train"][-1]) and np.array_equal(estart, first.preds["eval"][-1]), "the walk is the predict path's"
    for name, value in metric_params("quantile", 1.0, 0.95):
        b.set_param(name, value)
    got2, trees2 = grown(torch_cuda, tmp_path, "sampled", (), x, y, w, cuts, ev, True, b=b, **dict(kw, max_depth=3))
    second = M.MetricAudit("quantile", trees2, *T.sets_of("sampled", x, y, w, ev, start, estart), alpha=0.95)
    assert second.violations(got2, 2) == []
    assert len(trees2) == 2 and second.defined["train"][0] != first.defined["train"][0]
    T.conditions(second)
    done(b, [d, ed])


# ---- 5. the stop rule on the library's own curve ----

@pytest.mark.parametrize("case", M.STOP_CASES, ids=M.case_id)
def test_the_stop_rule_over_the_audited_sums(torch_cuda, tmp_path, case):
    kind, metric, slope, alpha, patience = case
    x, y, w, cuts, ev = T.inputs()
    kw = T.kind_hyper(kind, rounds=12, max_depth=3 if kind == "weighted" else 10)
    got, audit = audited(torch_cuda, tmp_path, case, x, y, w, cuts, ev, patience % 2 == 0, patience=patience, truth=False, **kw)
    assert audit.violations(got, 12, patience) == [], M.case_id(case)
    assert (got["rounds_run"], got["best_round"]) == M.stop_rule(audit.sums["eval"], 12, patience)
    if (kind, metric, patience) == ("weighted", "rmse", 2):
        assert 0 < got["best_round"] < got["rounds_run"] < 12, "the best round strictly inside"


def test_a_held_out_set_that_only_gets_worse_keeps_no_tree(torch_cuda, tmp_path):
    x, y, w, cuts, ev = T.inputs()
    case = ("weighted", "mae", 1.0, 0.5, 2)
    got, audit = audited(torch_cuda, tmp_path, case, x, y, w, cuts, T.mirrored(ev), False, patience=2, truth=False,
                         **T.kind_hyper("weighted", rounds=12, max_depth=3))
    assert audit.violations(got, 12, 2) == []
    assert (got["rounds_run"], got["best_round"], got["nodes_added"]) == (2, 0, 0)
