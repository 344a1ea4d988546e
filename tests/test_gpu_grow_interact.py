""""ohx_interaction_constraints" on the GPU (csrc/grow_interact.hip, through XGBoosterSetParam and interaction_constraints=
of the Python binding).  Models are compared byte for byte in all three formats, every array of every new tree bit for bit,
both metric arrays with ==, and nodes_added, rounds_run and best_round as integers.

The expected values are the restatement's (tests/grow_interact_support.py, written from the header) and, where the header
states an equality, another call on a twin booster.  The model of every case has no tree, so the margin a restatement
starts from is the model's base.  What a case is meant to reach - a tree that the groups change, a level beyond 7, more
open nodes than a batch holds - is asserted from the restatement before the GPU is asked.  Every tree a test saves is
audited for C2 from its saved bytes, independently of the restatement."""
import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_deep_support as D
from tests import grow_interact_support as I
from tests import grow_support as G
from tests.test_gpu_grow import held, same_new_trees
from tests.test_gpu_grow_eval import same_result, saved
from tests.test_gpu_grow_objective import NAN, booster as booster_of, call, done, same_arrays
from tests.test_grow_interact_cpu import c_call

pytestmark = pytest.mark.gpu

NAME = "ohx_interaction_constraints"
F32 = np.float32
N, SEED, HELD = 4097, 351, 400
SAMPLING = dict(subsample=0.7, colsample_bytree=0.75, seed=13)
GROUPS = {"two groups": I.TWO_GROUPS, "overlap": I.OVERLAP, "singletons": I.SINGLETONS}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def booster(params=()):
    return booster_of(params, nfeat=I.NFEAT)


def kw_of(kind, depth, rounds=2, **more):
    kw = dict(eta=0.125, reg_lambda=1.0, min_child_weight=0.0, max_depth=depth, rounds=rounds, **more)
    if "sampled" in kind:
        kw.update(SAMPLING)
    return kw


def restated(groups, kind, depth, n=N, seed=SEED, held_out=HELD, **more):
    s = SAMPLING if "sampled" in kind else {}
    return I.restated(tuple(groups), n, seed, depth, held_out=held_out, subsample=s.get("subsample", 1.0),
                      colsample=s.get("colsample_bytree", 1.0), draw_seed=s.get("seed", 0), **more)


def expected_images(tmp_path, want_trees):
    """The bytes, in all three formats, of a model that holds the restated trees."""
    empty = booster()
    other = capi.Booster(model_buffer=G.with_trees(held(empty, tmp_path, "empty.json")[1], want_trees))
    out = saved(other, tmp_path)
    empty.free()
    other.free()
    return out


def check(torch, tmp_path, kind, want, x, y, w, cuts, ev, params, groups, what, device=False, **kw):
    """One call on a fresh booster against the restatement, and C2 by the auditor on the saved bytes -> (result, images)."""
    b = booster(params)
    got, mats = call(torch, b, kind, x, y, w, cuts, ev, device=device, **kw)
    same_result(got, want, what)
    same_new_trees(held(b, tmp_path)[0], want["trees"], 0, what)
    images = saved(b, tmp_path)
    done(b, mats)
    assert images == expected_images(tmp_path, want["trees"]), (what, "the bytes of a model that holds the restated trees")
    for image in images:
        assert I.violations(image, groups, I.NFEAT) == [], (what, "C2")
    return got, images


# ---- 1, 2. every kind, both forms, against the restatement and the auditor ----

CASES = (("weighted", 3, False), ("weighted", 8, True), ("deep", 10, False), ("sampled", 6, True), ("deep_sampled", 10, False))


@pytest.mark.parametrize("name", tuple(GROUPS))
@pytest.mark.parametrize("kind,depth,device", CASES, ids=[f"{k}-{d}" for k, d, _ in CASES])
def test_constrained_trees_against_the_restatement(torch_cuda, tmp_path, kind, depth, device, name):
    groups = GROUPS[name]
    x, y, w, cuts, ev, want = restated(groups, kind, depth)
    *_, free = restated((), kind, depth)
    assert I.violations(free["all_trees"], groups, I.NFEAT), "the same call without the parameter violates C2"
    assert I.violations(want["all_trees"], groups, I.NFEAT) == [] and len(want["all_trees"]) == 2
    if depth > 8:
        assert any(D.depth_of(t) > 8 and D.levels(t)[8][1] > 0 for t in want["all_trees"]), "level 8 splits on the sets level 7 wrote"
    if name == "singletons":
        assert all(len(set(t["feature"][t["left"] >= 0].tolist())) == 1 for t in want["trees"]), "C3"
    what = f"{kind} at depth {depth}, {name}"
    kw = kw_of(kind, depth)
    # the one form by XGBoosterSetParam, the other by the keyword of the binding: the same bytes
    _, images = check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, ((NAME, I.text(groups)),), groups, what, device=device, **kw)
    _, other = check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, (), groups, what + ", the other form", device=not device,
                     interaction_constraints=[list(g) for g in groups], **kw)
    assert other == images


def test_the_call_without_the_parameter_violates_c2(torch_cuda, tmp_path):
    x, y, w, cuts, ev = I.inputs(N, SEED, 64, HELD)
    b = booster()
    got, mats = call(torch_cuda, b, "weighted", x, y, w, cuts, ev, **kw_of("weighted", 8))
    images = saved(b, tmp_path)
    done(b, mats)
    for image in images:
        assert I.violations(image, I.TWO_GROUPS, I.NFEAT), "a free tree mixes the groups"


# ---- 3. deep levels with more open nodes than a batch holds ----

def test_constrained_with_more_open_nodes_than_a_batch_holds(torch_cuda, tmp_path):
    """Depth 12, one round.  24 000 rows leave 806 open nodes at level 11 under two groups; 96 000 leave 1286."""
    n = 96000
    x, y, w, cuts, _, want = I.restated(I.TWO_GROUPS, n, SEED + 2, 12, rounds=1)
    assert max(o for o, _ in D.levels(want["trees"][0])[:12]) > synth.grow_deep_batch() == 1024, "a level of two batches"
    check(torch_cuda, tmp_path, "deep", want, x, y, w, cuts, None, ((NAME, I.text(I.TWO_GROUPS)),), I.TWO_GROUPS, "deep, two batches",
          **kw_of("deep", 12, rounds=1))


# ---- 4. composition ----

COMPOSED = {
    "monotone": (dict(constraints=(1, 0, -1)), (("ohx_monotone_constraints", "(1,0,-1)"),), {}),
    "alpha and step": (dict(alpha=0.5, m=0.5), (("ohx_reg_alpha", "0.5"), ("ohx_max_delta_step", "0.5")), {}),
    "pseudohuber": (dict(objective="pseudohuber"), (("ohx_objective", "pseudohuber"), ("ohx_huber_slope", "1.0")), {}),
    "mae and patience": (dict(metric="mae", patience=1, rounds=4), (("ohx_eval_metric", "mae"),), dict(patience=1, rounds=4)),
}


@pytest.mark.parametrize("name", tuple(COMPOSED))
def test_composition_against_the_restatement(torch_cuda, tmp_path, name):
    more, params, call_kw = COMPOSED[name]
    kind, depth = ("deep", 10) if name == "monotone" else ("weighted", 6)
    x, y, w, cuts, ev, want = restated(I.TWO_GROUPS, kind, depth, **more)
    *_, free = restated((), kind, depth, **more)
    assert I.violations(free["all_trees"], I.TWO_GROUPS, I.NFEAT) and want["nodes_added"] > 20
    if name == "monotone":
        *_, unbound = restated(I.TWO_GROUPS, kind, depth)
        assert not I.M.same_trees(want["all_trees"], unbound["all_trees"]), "the monotone constraints change a tree"
    check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, params + ((NAME, I.text(I.TWO_GROUPS)),), I.TWO_GROUPS, name,
          device=name in ("monotone", "pseudohuber"), **dict(kw_of(kind, depth), **call_kw))


# ---- 5. two calls on one handle: nothing stale is read from the sets ----

def test_a_second_call_under_other_groups_equals_a_fresh_handle(torch_cuda, tmp_path):
    x, y, w, cuts, ev, first = restated(I.TWO_GROUPS, "weighted", 8)
    other_groups = ((0, 3), (1, 2, 4, 5))
    b = booster(((NAME, I.text(I.TWO_GROUPS)),))
    got, mats = call(torch_cuda, b, "weighted", x, y, w, cuts, ev, **kw_of("weighted", 8))
    same_result(got, first, "the first call")
    start = saved(b, tmp_path)
    # the second call on the first's forest, and the same on a fresh handle that loads that forest
    fresh = capi.Booster(model_buffer=start[0])
    results = []
    for bb in (b, fresh):
        bb.set_param(NAME, I.text(other_groups))
        d = capi.DMatrix(x, missing=NAN)
        results.append(bb.boost_trees_weighted(d, y, cuts, weights=w, **kw_of("weighted", 3)))
        d.free()
    same_arrays(results[0], results[1], "the second call")
    images = saved(b, tmp_path)
    assert images == saved(fresh, tmp_path) and images != start
    assert results[0]["nodes_added"] > 8
    for image in images:
        assert I.violations(image, other_groups, I.NFEAT, first=2) == [], "the second call's trees under its own groups"
        assert I.violations(image, I.TWO_GROUPS, I.NFEAT, first=2), "they mix the first call's groups: x0 with x3"
    fresh.free()
    done(b, mats)


# ---- 6. C1 ----

@pytest.mark.parametrize("kind,depth", (("weighted", 6), ("deep_sampled", 10)))
def test_inactive_constraints_are_the_default(torch_cuda, tmp_path, kind, depth):
    x, y, w, cuts, ev = I.inputs(N, SEED + 3, 64, HELD)
    results, images = [], []
    for values in ((), ("[]",), ("[[5, 4, 3, 2, 1, 0]]",), ("[[0,1],[0,1,2,3,4,5]]",), (I.text(I.TWO_GROUPS), "[]"), (I.text(I.TWO_GROUPS),)):
        b = booster()
        for v in values:
            b.set_param(NAME, v)
        got, mats = call(torch_cuda, b, kind, x, y, w, cuts, ev, **kw_of(kind, depth))
        results.append(got)
        images.append(saved(b, tmp_path))
        done(b, mats)
    for k in (1, 2, 3, 4):
        same_arrays(results[k], results[0], (kind, k))
        assert images[k] == images[0], (kind, k)
    assert images[5] != images[0], "the active groups change the trees"


# ---- 7. C4 ----

@pytest.mark.parametrize("kind,depth", (("weighted", 8), ("deep", 10)))
def test_row_order_and_the_grid_change_nothing(torch_cuda, tmp_path, kind, depth):
    x, y, w, cuts, ev, want = restated(I.OVERLAP, kind, depth)
    params = ((NAME, I.text(I.OVERLAP)),)
    _, images = check(torch_cuda, tmp_path, kind, want, x, y, w, cuts, ev, params, I.OVERLAP, kind, **kw_of(kind, depth))
    order = np.random.default_rng(SEED + 4).permutation(N)
    b = booster(params)
    got, mats = call(torch_cuda, b, kind, np.ascontiguousarray(x[order]), y[order], w[order], cuts, ev, grid=True, **kw_of(kind, depth))
    same_result(got, want, kind + ", permuted")
    assert saved(b, tmp_path) == images, "permuted rows on a grid"
    done(b, mats)


# ---- 8. refusals ----

ENTRIES = ("OHXBoosterBoostTreesWeighted", "OHXBoosterBoostTreesSampled", "OHXBoosterBoostTreesDeep", "OHXBoosterBoostTreesDeepSampled")
COUNTS = ("OHXBoosterBoostTrees", "OHXBoosterBoostTreesEval")


def test_refusals_leave_the_forest_and_the_outputs_alone(torch_cuda, tmp_path):
    """Every refusal through the C interface itself, in both forms, on real matrices with every output array poisoned
    (c_call asserts that none was written), and the forest's bytes afterwards."""
    x, y, w, cuts, ev = I.inputs(N, SEED + 5, 64, HELD)
    b = booster()
    d = capi.DMatrix(x, missing=NAN)
    b.boost_trees_weighted(d, y, cuts, weights=w, **kw_of("weighted", 3))      # a forest to leave alone
    before = saved(b, tmp_path)
    tx, ty = torch_cuda.from_numpy(x).cuda(), torch_cuda.from_numpy(y).cuda()
    dd = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=N, ncol=I.NFEAT, missing=NAN)
    torch_cuda.cuda.synchronize()

    def refused(base, *said):
        """Both forms of one entry point: -1, no output written, and a message that says every word of `said`."""
        for name, mat, labels in ((base, d.handle, y.ctypes.data), (base + "Device", dd.handle, ty.data_ptr())):
            rc, msg = c_call(b, name, I.NFEAT, dmat=mat, labels=labels, nlabel=N)
            assert rc == -1 and all(word in msg for word in said + (NAME, "nothing was enqueued")), (name, msg)

    # an id equal to num_feature: every boost call
    b.set_param(NAME, "[[0, 6]]")
    for base in ENTRIES + COUNTS:
        refused(base)
    assert saved(b, tmp_path) == before, "an id that is no feature"
    # the two calls that keep row counts
    b.set_param(NAME, I.text(I.TWO_GROUPS))
    for base in COUNTS:
        refused(base, "OHXBoosterBoostTreesWeighted")
    assert saved(b, tmp_path) == before, "the calls that keep row counts"
    # the level and node fractions, where they take a feature away
    for fraction in ("ohx_colsample_bylevel", "ohx_colsample_bynode"):
        b.set_param(fraction, "0.5")
        for base in ("OHXBoosterBoostTreesSampled", "OHXBoosterBoostTreesDeepSampled"):
            refused(base, fraction)
        b.set_param(fraction, "1")
    assert saved(b, tmp_path) == before, "the fractions"
    # quantile (the Deep calls refuse that objective themselves)
    b.set_param("ohx_objective", "quantile")
    for base in ("OHXBoosterBoostTreesWeighted", "OHXBoosterBoostTreesSampled"):
        refused(base, "quantile")
    b.set_param("ohx_objective", "squarederror")
    assert saved(b, tmp_path) == before, "quantile"
    # the refit chooses no split and is unaffected; a valid call follows
    b.refit_leaves(d, y)
    before = saved(b, tmp_path)
    got = b.boost_trees_weighted(d, y, cuts, weights=w, **kw_of("weighted", 3))
    assert got["nodes_added"] > 0 and saved(b, tmp_path) != before, "a valid call after the refusals"
    done(b, [d, dd])
