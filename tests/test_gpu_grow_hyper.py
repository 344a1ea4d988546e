"""The three split policies of boosting on the GPU (csrc/grow_pairs.hip, grow_reg.hip, grow_mono.hip) away from the one point
of gamma, lambda, min_child_weight and eta at which test_gpu_grow_objective.py, test_gpu_grow_reg.py and test_gpu_grow_mono.py
grow their trees: gamma > 0, min_child_weight > 0 under fractional hessian sums, lambda = 0, eta 1 and 1/32, and two
combinations, over the four kinds, both forms and pseudo-Huber alone, regularised and constrained
(tests/grow_audit_support.py lists the cases).  Every array of every new tree, nodes_added, rounds_run and best_round are
compared as integers or bit for bit, both metric arrays with ==, and the model byte for byte in all three formats with a
model that holds the restated trees.

The expected values are the restatements' (tests/grow_objective_support.py, grow_reg_support.py, grow_mono_support.py).  What
a case is meant to reach - a level where gamma closes a node beside one that splits, a node closed by Hd < 2 min_child_weight,
a split that min_child_weight moves, level 8 - is asserted from the restatement before the GPU is asked.  A second check does
not share the restatements' origin: the exact audit of tests/grow_audit_support.py over the trees the library grew, with the
pairs of a round made from the margins of the library's own earlier trees.  Left out here and found in
tests/test_gpu_grow_audit.py: squared error off the defaults (the inline kernels, the plain and the Eval call among them),
and the audit of the bagged kinds and of the node sets of column sampling by level and by node."""
import ctypes as C

import numpy as np
import pytest

from quickchem_amd import capi
from tests import grow_audit_support as A
from tests import grow_support as G
from tests.test_gpu_grow import held, same_new_trees
from tests.test_gpu_grow_eval import same_result, saved
from tests.test_gpu_grow_mono import params_of
from tests.test_gpu_grow_objective import NAN, booster, call, done

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def grow(torch, tmp_path, kind, policy, setting, x, y, w, cuts, ev, device):
    """One call on a booster without trees -> (the result, the new trees, the three images)."""
    alpha, m, cons = A.POLICIES[policy]
    kw = A.hyper(kind, setting)
    if device:     # the device form, its parameters set by XGBoosterSetParam
        b = booster(params_of(cons, "pseudohuber", alpha, m), nfeat=A.NFEAT)
    else:          # the host form, by the keyword arguments of the binding
        b = booster(nfeat=A.NFEAT)
        kw.update(objective="pseudohuber", huber_slope=A.SLOPE, reg_alpha=alpha, max_delta_step=m, monotone_constraints=cons)
    got, mats = call(torch, b, kind, x, y, w, cuts, ev, device=device, **kw)
    trees, images = held(b, tmp_path)[0], saved(b, tmp_path)
    done(b, mats)
    return got, trees, images


def expected_images(tmp_path, want_trees):
    """The three images of a booster loaded from the empty model's JSON with the restated trees written into it."""
    empty = booster(nfeat=A.NFEAT)
    other = capi.Booster(model_buffer=G.with_trees(held(empty, tmp_path, "empty.json")[1], want_trees))
    out = saved(other, tmp_path)
    empty.free()
    other.free()
    return out


# ---- 1. off the defaults, against the restatement ----

@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
def test_off_default_hyper_parameters_against_the_restatement(torch_cuda, tmp_path, case):
    kind, form, policy, setting, seed = case
    want = A.reaches(kind, policy, setting, seed)
    x, y, w, cuts, ev, _ = A.restated(kind, policy, setting, seed)
    got, trees, images = grow(torch_cuda, tmp_path, kind, policy, setting, x, y, w, cuts, ev, form == "device")
    same_result(got, want, A.case_id(case))
    same_new_trees(trees, want["trees"], 0, A.case_id(case))
    assert images == expected_images(tmp_path, want["trees"]), "the bytes of a model that holds the restated trees"
    # the other form: the same numbers and the same bytes
    got, _, other = grow(torch_cuda, tmp_path, kind, policy, setting, x, y, w, cuts, ev, form != "device")
    same_result(got, want, A.case_id(case) + ", the other form")
    assert other == images, "the other form"


# ---- 2. the refusal that only lambda 0 reaches ----

REFUSED = "a gradient pred - label is not finite or reaches 256"        # (the training rows' message, not the held-out rows')
ENTRIES = {("weighted", False): "OHXBoosterBoostTreesWeighted", ("weighted", True): "OHXBoosterBoostTreesWeightedDevice",
           ("deep", False): "OHXBoosterBoostTreesDeep"}


@pytest.mark.parametrize("kind,device", tuple(ENTRIES))
def test_a_margin_thrown_out_of_range_at_lambda_0_refuses_the_whole_call(torch_cuda, tmp_path, kind, device):
    """Pseudo-Huber at lambda 0, min_child_weight 0, no step, on a forest of one tree: a child of hessian sum near 1e-5 gets a
    leaf that throws a margin past 256, and the header refuses the call whole: -1 and "label", the forest's bytes and the
    caller's arrays and counters as they were.  Under ohx_max_delta_step = 0.5 the same call succeeds."""
    torch = torch_cuda
    x, y, w, cuts, ev, first, again = A.refusal_case(kind)
    with pytest.raises(ValueError, match="^label: a residual is not finite or reaches 256"):
        again(0.0)
    want = again(0.5)
    assert want["nodes_added"] > 150 and want["rounds_run"] == 2
    kw = A.hyper(kind, dict(reg_lambda=0.0))
    n, en = len(y), len(ev[2])
    b = booster((("ohx_objective", "pseudohuber"),), nfeat=A.NFEAT)
    if device:
        tx, ty, tw = (torch.from_numpy(v).cuda() for v in (x, y, w))
        tex, tey, tew = (torch.from_numpy(v).cuda() for v in (ev[0], ev[2], ev[3]))
        torch.cuda.synchronize()
        d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=n, ncol=A.NFEAT, missing=NAN)
        ed = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=en, ncol=A.NFEAT, missing=NAN)
        rows = (ty.data_ptr(), tw.data_ptr(), n, ed.handle, tey.data_ptr(), tew.data_ptr(), en)
        method = getattr(b, "boost_trees_" + kind + "_device")
        args, more = (d, ty.data_ptr(), n, cuts), dict(weights_ptr=tw.data_ptr(), eval_set=(ed, tey.data_ptr(), en, tew.data_ptr()))
    else:
        d, ed = capi.DMatrix(x, missing=NAN), capi.DMatrix(ev[0], missing=NAN)
        rows = (y.ctypes.data, w.ctypes.data, n, ed.handle, ev[2].ctypes.data, ev[3].ctypes.data, en)
        method = getattr(b, "boost_trees_" + kind)
        args, more = (d, y, cuts), dict(weights=w, eval_set=(ed, ev[2], ev[3]))
    # the forest to leave alone
    got = method(*args, **more, **dict(kw, reg_lambda=1.0, rounds=1, max_depth=3))
    same_result(got, first, "the first tree")
    same_new_trees(held(b, tmp_path)[0], first["trees"], 0, "the first tree")
    before = saved(b, tmp_path)
    # through the C interface itself, the outputs preset
    ptr, vals = b._cuts(cuts)
    train, evals = np.full(3, -7.0), np.full(3, -7.0)
    run, best, added = C.c_int32(-7), C.c_int32(-7), C.c_uint64(77)
    rc = getattr(b.lib, ENTRIES[kind, device])(b.handle, d.handle, *rows, ptr.ctypes.data, vals.ctypes.data, kw["rounds"], kw["max_depth"],
                                               kw["eta"], 0.0, 0.0, 0.0, 0, train.ctypes.data, evals.ctypes.data, C.byref(run),
                                               C.byref(best), C.byref(added), *((None,) if device else ()))
    assert rc == -1
    with pytest.raises(capi.OhxError, match=REFUSED):
        capi.check(b.lib, rc)
    assert np.all(train == -7.0) and np.all(evals == -7.0) and run.value == -7 and best.value == -7 and added.value == 77
    assert saved(b, tmp_path) == before, "the refused call left the forest alone"
    # and by the binding
    with pytest.raises(capi.OhxError, match=REFUSED):
        method(*args, **more, **kw)
    assert saved(b, tmp_path) == before, "the refused call left the forest alone"
    # under a step the same call succeeds, on top of the forest
    b.set_param("ohx_max_delta_step", "0.5")
    got = method(*args, **more, **kw)
    same_result(got, want, "under a step")
    same_new_trees(held(b, tmp_path)[0], want["trees"], 1, "under a step")
    done(b, [d, ed])


# ---- 3. the exact audit of what the library grew ----

@pytest.mark.parametrize("case", A.AUDITED, ids=A.case_id)
def test_the_trees_the_library_grew_pass_the_exact_audit(torch_cuda, tmp_path, case):
    """Each policy at the combination, on the LDS path and on the deep one, in the form that the comparison above does not
    take.  The audit knows the rows, the labels and the library's trees, not the restatement: a round's pairs come from the
    margins of the library's earlier trees, walked on the host.  The constrained trees are monotone on the sweeps; their
    free twins, the pairs cases, are not."""
    kind, form, policy, setting, seed = case
    x, y, w, cuts, ev, want = A.restated(kind, policy, setting, seed)
    got, trees, _ = grow(torch_cuda, tmp_path, kind, policy, setting, x, y, w, cuts, ev, form == "host")
    assert got["nodes_added"] == sum(len(t["left"]) for t in trees) and len(trees) == A.ROUNDS
    for r, a in enumerate(A.audits(kind, policy, setting, x, y, w, cuts, trees)):
        assert a.violations() == [], (A.case_id(case), "tree", r)
        assert sum(1 for p in a.order if trees[r]["left"][p] >= 0) >= 10, "a tree with splits to audit"
        bent = A.sweep_violations(trees[r], x, cuts, A.CONSTRAINTS)
        if A.POLICIES[policy][2]:
            assert bent == 0, (A.case_id(case), "tree", r)
        elif policy == "pairs":
            assert bent > 0, "the free twin is not monotone: the sweep bites"
    same_new_trees(trees, want["trees"], 0, A.case_id(case))
