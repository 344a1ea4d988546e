"""Boosters with several output groups on the GPU, against their decomposition: column g of the margins is, bit for bit,
the margin of the single-group booster made of group g's trees in file order (which the oracle matches too), whatever
the kernel, the form, the missing marker, ntree_limit and the batch size; the transforms, the leaf ids, contributions
and interactions are checked the same way, and scikit-learn's 3-class GradientBoostingClassifier is an outside check."""
import json

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import helpers
from tests import output_groups_support as OG

pytestmark = pytest.mark.gpu

G3 = 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def img(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def booster(image, kernel="auto"):
    b = capi.Booster(model_buffer=img(image))
    if kernel != "auto":
        b.set_param("ohx_kernel", kernel)
    return b


def predict_host(image, rows, missing, option_mask=1, ntree_limit=0, kernel="auto", grid=None):
    b = booster(image, kernel)
    d = capi.DMatrix(rows, missing=missing)
    if grid is not None:
        d.set_grid(grid[0], grid[1], 0)
    out = b.predict(d, option_mask=option_mask, ntree_limit=ntree_limit)
    d.free()
    b.free()
    return out


def predict_device(torch, image, rows, missing, option_mask=1, ntree_limit=0, kernel="auto", grid=None, width=None):
    b = booster(image, kernel)
    t = torch.from_numpy(rows).cuda()
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=len(rows), ncol=rows.shape[1], missing=missing)
    if grid is not None:
        d.set_grid(grid[0], grid[1], 0)
    out = torch.full((len(rows) * width,), float("nan"), dtype=torch.float32, device="cuda")
    b.predict_device(d, out.data_ptr(), option_mask=option_mask, ntree_limit=ntree_limit)
    torch.cuda.synchronize()
    b.check()
    got = out.cpu().numpy()
    d.free()
    b.free()
    return got


def expected_margins(image, info, G, rows, missing, ntree_limit=0, kernel="auto", grid=None, oracle=True):
    """[nrow][G] from the single-group boosters (and the oracle on each of them)."""
    cnt, _ = OG.group_counts(info, G, ntree_limit)
    out = np.empty((len(rows), G), dtype=np.float32)
    for g in range(G):
        sub = OG.sub_json(image, info, g)
        if sub is None or cnt[g] == 0:
            out[:, g] = OG.base_margin(image)
            continue
        m = predict_host(sub, rows, missing, 1, cnt[g], kernel, grid)
        if oracle:
            want = helpers.oracle_predict(synth.convert_model(sub, "binary"), rows, missing, option_mask=1,
                                          ntree_limit=cnt[g])
            assert np.array_equal(helpers.bits(m), helpers.bits(want)), "group %d: sub-booster against the oracle" % g
        out[:, g] = m
    return out


@pytest.fixture(scope="module")
def irregular():
    rows = S.rows_for(11, [], 64, float("nan"), tie_fraction=0.0)
    image, trees, info = OG.make_multi(4242, 31, G3, "irregular", rows=rows)
    return image, trees, info


@pytest.fixture(scope="module")
def with_empty():
    image, trees, info = OG.make_multi(4343, 20, 4, "one_empty")
    return image, trees, info


@pytest.mark.parametrize("kernel", ["auto", "ring", "super2", "packed2", "wide"])
@pytest.mark.parametrize("nrow", [1, 63, 65, 10000])
@pytest.mark.parametrize("missing", [float("nan"), -999.0])
def test_margins_decompose_by_group(irregular, kernel, nrow, missing):
    image, trees, info = irregular
    rows = S.rows_for(nrow + 7, trees, nrow, missing)
    got = predict_host(image, rows, missing, 1, 0, kernel)
    assert got.shape == (nrow, G3)
    want = expected_margins(image, info, G3, rows, missing, 0, kernel, oracle=(kernel == "auto"))
    assert np.array_equal(helpers.bits(got), helpers.bits(want))


@pytest.mark.parametrize("kernel", ["auto", "ring", "packed2"])
@pytest.mark.parametrize("ntree_limit", [0, 1, 4, 1000])
def test_device_form_and_ntree_limit(torch_cuda, irregular, kernel, ntree_limit):
    image, trees, info = irregular
    rows = S.rows_for(5, trees, 2000, float("nan"))
    got = predict_device(torch_cuda, image, rows, float("nan"), 1, ntree_limit, kernel, width=G3).reshape(-1, G3)
    host = predict_host(image, rows, float("nan"), 1, ntree_limit, kernel)
    assert np.array_equal(helpers.bits(got), helpers.bits(host))
    want = expected_margins(image, info, G3, rows, float("nan"), ntree_limit, kernel)
    assert np.array_equal(helpers.bits(got), helpers.bits(want))


def test_an_empty_group_holds_the_base_margin(with_empty):
    image, trees, info = with_empty
    rows = S.rows_for(9, trees, 700, -999.0)
    got = predict_host(image, rows, -999.0, 1)
    assert got.shape == (700, 4)
    assert np.array_equal(helpers.bits(got[:, 1]), helpers.bits(np.full(700, OG.base_margin(image), np.float32)))
    assert np.array_equal(helpers.bits(got), helpers.bits(expected_margins(image, info, 4, rows, -999.0)))


def test_a_row_does_not_depend_on_its_batch(irregular):
    image, trees, info = irregular
    rows = S.rows_for(21, trees, 3000, float("nan"))
    whole = predict_host(image, rows, float("nan"), 1)
    parts = np.concatenate([predict_host(image, rows[a:a + 61], float("nan"), 1) for a in range(0, 3000, 61)])
    assert np.array_equal(helpers.bits(whole), helpers.bits(parts))


@pytest.mark.parametrize("with_grid", [True, False])
def test_big_batches_ring_deferred_rows_and_clustering(irregular, with_grid):
    """>= 262 144 rows: with a grid the ring kernel with rows deferred to a second launch, without one (rows shuffled)
    the clustering pass in front of the walk."""
    grid = (64, 64, 64)
    rows = synth.rows_cpu(grid, 0, 64 * 64 * 64)
    image, trees, info = OG.make_multi(77, 30, G3, "round_robin", rows=rows[::97])
    rng = np.random.default_rng(3)
    rows = rows.copy()
    rows[rng.random(rows.shape) < 2e-4] = synth.XX_MISS
    if not with_grid:
        rows = np.ascontiguousarray(rows[rng.permutation(len(rows))])
    g = grid if with_grid else None
    got = predict_host(image, rows, synth.XX_MISS, 1, 0, "auto", g)
    want = expected_margins(image, info, G3, rows, synth.XX_MISS, 0, "auto", g, oracle=False)
    assert np.array_equal(helpers.bits(got), helpers.bits(want))
    sub0 = OG.sub_json(image, info, 0)
    assert np.array_equal(helpers.bits(want[:, 0]),
                          helpers.bits(helpers.oracle_predict(synth.convert_model(sub0, "binary"), rows, synth.XX_MISS,
                                                                     option_mask=1)))


def float64_softmax(m):
    m = m.astype(np.float64)
    e = np.exp(m - m.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("G", [3, 5])
def test_softprob_is_the_softmax_of_the_margins(G):
    """Bound: 8 float32 ulp of the float64 softmax of the returned margins (expf, a double sum, a float divide)."""
    image, trees, info = OG.make_multi(600 + G, 4 * G, G, "round_robin")
    rows = S.rows_for(2, trees, 5000, float("nan"))
    margins = predict_host(image, rows, float("nan"), 1)
    prob = predict_host(image, rows, float("nan"), 0)
    assert prob.shape == (5000, G)
    ref = float64_softmax(margins)
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(prob.astype(np.float64) - ref) <= 8 * ulp)
    assert np.all(np.abs(prob.astype(np.float64).sum(axis=1) - 1.0) <= 1e-6)


def test_softmax_is_the_first_maximal_margin_ties_included():
    """Groups 0 and 2 hold the same trees: every row ties between them unless group 1 is larger."""
    image, trees = S.make_booster(31, 6)
    doc = json.loads(image)
    model = doc["learner"]["gradient_booster"]["model"]
    t = model["trees"]
    model["trees"] = [dict(x, id=i) for i, x in enumerate(t[:3] + t[3:] + t[:3])]
    info = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    model["gbtree_model_param"]["num_trees"] = "9"
    tied = OG.multi_json(json.dumps(doc).encode(), info, 3, "multi:softmax")
    rows = S.rows_for(4, trees, 3000, float("nan"))
    margins = predict_host(tied, rows, float("nan"), 1)
    assert np.array_equal(helpers.bits(margins[:, 0]), helpers.bits(margins[:, 2]))
    cls = predict_host(tied, rows, float("nan"), 0)
    assert cls.shape == (3000,)
    assert np.array_equal(cls, np.argmax(margins, axis=1).astype(np.float32))
    assert np.any(cls == 0) and not np.any(cls == 2)


def test_multi_target_regression_value_is_the_margin():
    image, trees, info = OG.make_multi(808, 12, 3, "blocked", objective="reg:squarederror", multi_target=True)
    rows = S.rows_for(8, trees, 999, float("nan"))
    value = predict_host(image, rows, float("nan"), 0)
    assert value.shape == (999, 3)
    assert np.array_equal(helpers.bits(value), helpers.bits(predict_host(image, rows, float("nan"), 1)))
    assert np.array_equal(helpers.bits(value), helpers.bits(expected_margins(image, info, 3, rows, float("nan"))))


def test_other_objectives_are_still_refused_for_values():
    image, trees, info = OG.make_multi(809, 6, 2, "blocked", objective="binary:logistic")
    rows = S.rows_for(8, trees, 10, float("nan"))
    with pytest.raises(capi.OhxError, match="prediction transform"):
        predict_host(image, rows, float("nan"), 0)


@pytest.mark.parametrize("ntree_limit", [0, 2, 1000])
def test_leaf_ids_in_file_order(irregular, ntree_limit):
    image, trees, info = irregular
    rows = S.rows_for(13, trees, 500, float("nan"))
    got = predict_host(image, rows, float("nan"), 16, ntree_limit)
    cnt, L = OG.group_counts(info, G3, ntree_limit)
    assert got.shape == (500, L)
    for g in range(G3):
        cols = [t for t in range(L) if info[t] == g]
        if not cols:
            continue
        sub = predict_host(OG.sub_json(image, info, g), rows, float("nan"), 16, cnt[g]).reshape(500, cnt[g])
        assert np.array_equal(got[:, cols], sub)


def test_capture_of_a_multi_group_device_predict_is_refused(torch_cuda, irregular):
    torch = torch_cuda
    image, trees, info = irregular
    rows = torch.from_numpy(S.rows_for(1, trees, 256, float("nan"))).cuda()
    out = torch.zeros(256 * G3, dtype=torch.float32, device="cuda")
    b = booster(image)
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=256, ncol=27, missing=float("nan"))
    b.predict_device(d, out.data_ptr(), option_mask=1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="several output groups"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.predict_device(d, out.data_ptr(), option_mask=1, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    b.check()


# ---- contributions and interactions ----

@pytest.fixture(scope="module")
def contribs_case():
    image, trees, info = OG.make_multi(5151, 18, 4, "one_empty", contribs=True)
    return image, trees, info


@pytest.mark.parametrize("approximate", [False, True])
@pytest.mark.parametrize("nrow", [40, 3000])
def test_contributions_decompose_by_group(contribs_case, approximate, nrow):
    image, trees, info = contribs_case
    rows = S.rows_for(nrow, trees, nrow, -999.0)
    b = booster(image)
    got = b.predict_contribs(capi.DMatrix(rows, missing=-999.0), approximate=approximate)
    assert got.shape == (nrow, 4, 28)
    margins = predict_host(image, rows, -999.0, 1)
    for g in range(4):
        sub = OG.sub_json(image, info, g)
        if sub is None:
            assert np.all(got[:, g, :27] == 0) and np.all(got[:, g, 27] == OG.base_margin(image))
            continue
        want = booster(sub).predict_contribs(capi.DMatrix(rows, missing=-999.0), approximate=approximate)
        assert np.array_equal(helpers.bits(got[:, g]), helpers.bits(want))
        # local accuracy: the bound test_gpu_contribs.py states for these adversarial paths (float32 TreeSHAP)
        phi = got[:, g].astype(np.float64)
        assert np.all(np.abs(phi.sum(axis=1) - margins[:, g]) <= 1e-3 * (1.0 + np.abs(phi).sum(axis=1)))


@pytest.mark.parametrize("approximate", [False, True])
def test_interactions_decompose_by_group(contribs_case, approximate):
    image, trees, info = contribs_case
    rows = S.rows_for(3, trees, 70, float("nan"))
    got = booster(image).predict_interactions(capi.DMatrix(rows, missing=float("nan")), approximate=approximate)
    assert got.shape == (70, 4, 28, 28)
    for g in range(4):
        sub = OG.sub_json(image, info, g)
        if sub is None:
            continue
        want = booster(sub).predict_interactions(capi.DMatrix(rows, missing=float("nan")), approximate=approximate)
        assert np.array_equal(helpers.bits(got[:, g]), helpers.bits(want))


def test_contributions_device_form_is_the_host_form(torch_cuda, contribs_case):
    torch = torch_cuda
    image, trees, info = contribs_case
    rows = S.rows_for(17, trees, 300, float("nan"))
    b = booster(image)
    host = b.predict_contribs(capi.DMatrix(rows, missing=float("nan")))
    t = torch.from_numpy(rows).cuda()
    out = torch.full((300 * 4 * 28,), float("nan"), dtype=torch.float32, device="cuda")
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=300, ncol=27, missing=float("nan"))
    b.predict_contribs_device(d, out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(helpers.bits(out.cpu().numpy().reshape(300, 4, 28)), helpers.bits(host))


@pytest.mark.parametrize("approximate", [False, True])
def test_a_failed_allocation_leaves_no_error_behind(torch_cuda, approximate):
    """Three output groups: an output (and a block buffer) that cannot be allocated, 2**40 borrowed rows, is refused
    with a message before anything is launched, and the failure is forgotten with it - the next host call and the next
    device call on the caller's stream give the bits of the call before."""
    from tests import contribs_support as cs
    torch = torch_cuda
    rng = np.random.default_rng(34)
    js, _, _ = cs.random_booster(rng, 3, 4, 4, 0.1)
    image = OG.multi_json(js, [0, 1, 2], 3)
    rows = cs.random_rows(rng, 64, 4)
    b = booster(image)
    d = capi.DMatrix(rows, missing=-999.0)
    before = b.predict_contribs(d, approximate=approximate)
    assert before.shape == (64, 3, 5)
    t = torch.from_numpy(rows).cuda()
    huge = capi.DMatrix(device_ptr=t.data_ptr(), nrow=1 << 40, ncol=4, missing=-999.0)
    with pytest.raises(capi.OhxError):
        b.predict_contribs(huge, approximate=approximate)
    assert np.array_equal(helpers.bits(b.predict_contribs(d, approximate=approximate)), helpers.bits(before))
    out = torch.zeros((64, 3, 5), dtype=torch.float32, device="cuda")
    dd = capi.DMatrix(device_ptr=t.data_ptr(), nrow=64, ncol=4, missing=-999.0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.predict_contribs_device(dd, out.data_ptr(), approximate=approximate, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(before))


# ---- outside cross-check: scikit-learn's multi-class gradient boosting ----

def test_sklearn_three_class_gradient_boosting():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import GradientBoostingClassifier
    from tests.test_sklearn_crosscheck import transcribe
    grid = synth.GRIDS["C12"]
    rows = synth.rows_cpu(grid, 0, grid[0] * grid[1] * grid[2])
    rng = np.random.default_rng(5)
    train = rows[rng.choice(len(rows), 4000, replace=False)]
    score = np.log10(train[:, 4] + 1e-12) + 0.01 * train[:, 2] + 0.3 * rng.normal(size=len(train))
    y = np.digitize(score, np.quantile(score, [1 / 3, 2 / 3]))
    gbc = GradientBoostingClassifier(n_estimators=12, max_depth=6, learning_rate=0.3, init="zero", random_state=0)
    gbc.fit(train, y)
    rounds, K = gbc.estimators_.shape
    assert K == 3
    ests = [gbc.estimators_[i, k] for i in range(rounds) for k in range(K)]
    js, maps = transcribe(gbc, rows.shape[1], estimators=ests, base=0.0)
    image = OG.multi_json(js, [t % K for t in range(len(ests))], K, "multi:softprob")
    test = np.ascontiguousarray(rows[rng.choice(len(rows), 5000, replace=False)], dtype=np.float32)
    leaves = predict_host(image, test, float("nan"), 16)
    want_leaves = np.asarray(gbc.apply(test))                     # (nrow, rounds, K)
    for t, m in enumerate(maps):
        lut = np.full(max(m) + 1, -1, dtype=np.int64)
        for new, old in m.items():
            lut[new] = old
        assert np.array_equal(lut[leaves[:, t].astype(np.int64)], want_leaves[:, t // K, t % K].astype(np.int64))
    margins = predict_host(image, test, float("nan"), 1)
    np.testing.assert_allclose(margins, gbc.decision_function(test), rtol=1e-5, atol=1e-5)
    prob = predict_host(image, test, float("nan"), 0)
    np.testing.assert_allclose(prob, gbc.predict_proba(test), rtol=0, atol=1e-5)
