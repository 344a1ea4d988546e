"""What tests/test_gpu_grow_hyper.py and tests/test_gpu_grow_colsample.py leave out, on the GPU: squared error through the
inline kernels (csrc/grow.hip, grow_eval.hip, grow_weighted.hip, grow_sampled.hip, the inline histograms of grow_deep.hip)
and the level and node lists of csrc/grow_colsample.hip away from the few points of gamma, lambda, the child minimum and eta
at which the other files grow their trees; and the exact audit of tests/grow_audit_support.py over the calls it had not
reached: all six kinds under squared error, the two that count rows among them, the bag and the tree's list, and the node
sets, where the audit asks of the library's own tree whether a node's split is the best of the node's own columns and
whether a closed node had no candidate above gamma among them.

The cases are grow_audit_support's INLINE_CASES, COLSAMPLE_CASES and AUDITED_MORE.  The expected values are the existing
restatements'; what a case is meant to reach, and that its trees leave the audit enough to judge, is asserted from the
restatement before the GPU is asked (tests/test_grow_audit_cpu.py does the same without one)."""
import numpy as np
import pytest

from quickchem_amd import capi
from tests import grow_audit_support as A
from tests import grow_support as G
from tests.test_gpu_grow import held, same_new_trees
from tests.test_gpu_grow_colsample import DRAW_SEED, check_c2
from tests.test_gpu_grow_eval import same_result, saved
from tests.test_gpu_grow_hyper import expected_images
from tests.test_gpu_grow_mono import params_of
from tests.test_gpu_grow_objective import NAN, booster, call, done, same_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def call_counting(torch, b, kind, x, y, cuts, ev, device, **kw):
    """One plain or Eval call, by its own binding method -> (the result dict - of the plain call nodes_added alone - and the
    matrices to free)."""
    if device:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            tx, ty = torch.from_numpy(x).to("cuda"), torch.from_numpy(y).to("cuda")
            if ev is not None:
                tex, tey = torch.from_numpy(ev[0]).to("cuda"), torch.from_numpy(ev[2]).to("cuda")
        s.synchronize()
        d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=x.shape[0], ncol=x.shape[1], missing=NAN)
        ed = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=ev[0].shape[0], ncol=ev[0].shape[1], missing=NAN) if ev is not None else None
        if kind == "plain":
            got = dict(nodes_added=b.boost_trees_device(d, ty.data_ptr(), len(y), cuts, stream=s.cuda_stream, **kw))
        else:
            got = b.boost_trees_eval_device(d, ty.data_ptr(), len(y), cuts, eval_set=(ed, tey.data_ptr(), len(ev[2])), stream=s.cuda_stream, **kw)
    else:
        d = capi.DMatrix(x, missing=NAN)
        ed = capi.DMatrix(ev[0], missing=ev[1]) if ev is not None else None
        if kind == "plain":
            got = dict(nodes_added=b.boost_trees(d, y, cuts, **kw))
        else:
            got = b.boost_trees_eval(d, y, cuts, eval_set=(ed, ev[2]), **kw)
    return got, [m for m in (d, ed) if m is not None]


def grow(torch, tmp_path, case, x, y, w, cuts, ev, device, more=()):
    """One call of the case on a booster without trees -> (the result, the new trees, the three images).  An inline case
    sets no handle parameter (`more`: those a test adds).  The others set theirs by XGBoosterSetParam in the device form
    and by the keyword arguments of the binding in the host form."""
    kind, _, objective, policy, _, _, (bylevel, bynode) = case
    alpha, m, cons = A.POLICIES[policy]
    kw = A.case_hyper(case)
    nfeat = A.nfeat_of(case)
    if case in A.INLINE_CASES:
        b = booster(more, nfeat=nfeat)
    elif device:
        fractions = (("ohx_colsample_bylevel", repr(bylevel)), ("ohx_colsample_bynode", repr(bynode))) if case[6] != A.NO_FRACTIONS else ()
        b = booster(params_of(cons, objective, alpha, m) + fractions + tuple(more), nfeat=nfeat)
    else:
        b = booster(more, nfeat=nfeat)
        kw.update(objective=objective, huber_slope=A.SLOPE, reg_alpha=alpha, max_delta_step=m, monotone_constraints=cons)
        if case[6] != A.NO_FRACTIONS:
            kw.update(colsample_bylevel=bylevel, colsample_bynode=bynode)
    if kind in A.COUNT_KINDS:
        got, mats = call_counting(torch, b, kind, x, y, cuts, ev, device, **kw)
    else:
        got, mats = call(torch, b, kind, x, y, w, cuts, ev, device=device, **kw)
    trees, images = held(b, tmp_path)[0], saved(b, tmp_path)
    done(b, mats)
    return got, trees, images


def same_numbers(got, want, what):
    if "train_rmse" in got:
        same_result(got, want, what)
    else:
        assert got["nodes_added"] == want["nodes_added"], (what, got, want["nodes_added"])


def against_the_restatement(torch, tmp_path, case):
    """The case's form first, then the other: the same numbers, the same trees, the same bytes -> the trees."""
    want = A.reaches_more(case)
    x, y, w, cuts, ev, _ = A.restated_more(case)
    what = A.more_id(case)
    got, trees, images = grow(torch, tmp_path, case, x, y, w, cuts, ev, case[1] == "device")
    same_numbers(got, want, what)
    same_new_trees(trees, want["trees"], 0, what)
    assert images == expected_images_of(tmp_path, A.nfeat_of(case), want["trees"]), "the bytes of a model that holds the restated trees"
    got, _, other = grow(torch, tmp_path, case, x, y, w, cuts, ev, case[1] != "device")
    same_numbers(got, want, what + ", the other form")
    assert other == images, "the other form"
    return trees


def expected_images_of(tmp_path, nfeat, want_trees):
    """test_gpu_grow_hyper.expected_images, which is written for grow_audit_support.NFEAT features."""
    if nfeat == A.NFEAT:
        return expected_images(tmp_path, want_trees)
    empty = booster(nfeat=nfeat)
    other = capi.Booster(model_buffer=G.with_trees(held(empty, tmp_path, "empty.json")[1], want_trees))
    out = saved(other, tmp_path)
    empty.free()
    other.free()
    return out


# ---- 1. squared error off the defaults: the inline kernels against the restatements ----

@pytest.mark.parametrize("case", A.INLINE_CASES, ids=A.more_id)
def test_inline_off_default_against_the_restatement(torch_cuda, tmp_path, case):
    against_the_restatement(torch_cuda, tmp_path, case)


# ---- 2. the header's equality, off kind_kw's point ----

@pytest.mark.parametrize("case", tuple(c for c in A.INLINE_CASES if c[0] not in A.COUNT_KINDS and "combination" in c[4]), ids=A.more_id)
def test_squared_error_by_the_pair_kernels_off_default(torch_cuda, tmp_path, case):
    """"ohx_grow_pairs" = on leaves the bytes and the metric arrays of the inline call, at the combination."""
    x, y, w, cuts, ev, want = A.restated_more(case)
    inline, _, inline_bytes = grow(torch_cuda, tmp_path, case, x, y, w, cuts, ev, case[1] == "device")
    by_pairs, _, pair_bytes = grow(torch_cuda, tmp_path, case, x, y, w, cuts, ev, case[1] == "device", more=(("ohx_grow_pairs", "on"),))
    assert inline["nodes_added"] == want["nodes_added"] > 40
    same_arrays(by_pairs, inline, A.more_id(case))
    assert pair_bytes == inline_bytes, A.more_id(case)


# ---- 3. the level and the node lists off the defaults ----

@pytest.mark.parametrize("case", A.COLSAMPLE_CASES, ids=A.more_id)
def test_colsample_off_default_against_the_restatement(torch_cuda, tmp_path, case):
    kw = A.case_hyper(case)
    assert kw["seed"] == DRAW_SEED, "check_c2 draws with it"
    trees = against_the_restatement(torch_cuda, tmp_path, case)
    splits = sum(int(np.count_nonzero(np.asarray(t["left"]) >= 0)) for t in trees)
    assert check_c2(trees, A.nfeat_of(case), case[6][0], case[6][1], kw["colsample_bytree"]) == splits > 0


# ---- 4. the exact audit of what the library grew ----

@pytest.mark.parametrize("case", A.AUDITED_MORE, ids=A.more_id)
def test_the_trees_the_library_grew_pass_the_exact_audit(torch_cuda, tmp_path, case):
    """In the form that the comparisons above do not take first.  The audit knows the rows, the labels and the library's
    trees, not the restatement: a round's pairs come from the margins of the library's earlier trees, walked on the host."""
    x, y, w, cuts, ev, want = A.restated_more(case)
    got, trees, _ = grow(torch_cuda, tmp_path, case, x, y, w, cuts, ev, case[1] == "host")
    assert got["nodes_added"] == sum(len(t["left"]) for t in trees) and len(trees) == A.ROUNDS
    audits = A.audits_more(case, x, y, w, cuts, trees)
    for r, a in enumerate(audits):
        assert a.violations() == [], (A.more_id(case), "tree", r)
        assert sum(1 for p in a.order if trees[r]["left"][p] >= 0) >= 10, "a tree with splits to audit"
        if A.POLICIES[case[3]][2]:
            assert A.sweep_violations(trees[r], x, cuts, A.CONSTRAINTS) == 0, (A.more_id(case), "tree", r)
    assert sum(A.decided(a) for a in audits) >= 10, "splits at which a wrong choice would be reported"
    same_new_trees(trees, want["trees"], 0, A.more_id(case))
