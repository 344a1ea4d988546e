"""SHAP interaction values on the GPU (OHXBoosterPredictInteractions / ...Device, csrc/interactions.hip): exact mode
against the float64 Shapley interaction index, the float64 per-path reference and the CPU restatement; approximate
mode bit for bit against approximate contributions; the diagonal's float order over the contributions kernel's phi;
local accuracy, symmetry; every length class and the adversarial boosters; the edges of the launch shapes (each first
asking synth.interactions_plan which shape it gets); determinism across calls, batches, forms and shapes; the
refusals; a device move; and buffers kept apart from a captured predict's."""
import functools
import json

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import contribs_support as cs
from tests import helpers
from tests import interactions_support as isup

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0DEAD


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def oh20():
    """The synthetic OH recipe at 20 trees (depth <= 18, grown on C12): test_gpu_contribs.py's contribs_model."""
    return synth.make_model(num_trees=20, max_depth=18, sample_log2=16, min_leaf=2, grid=synth.GRIDS["C12"])


def device_form(torch, b, x, missing, approximate=False, ntree_limit=0, nrow=None):
    """The device form into a buffer with a canary behind the nrow * (F + 1)^2 floats it may write."""
    nrow = len(x) if nrow is None else nrow
    F1 = b.info()["num_feature"] + 1
    t = torch.from_numpy(np.ascontiguousarray(x if len(x) else np.zeros((1, x.shape[1]), np.float32))).cuda()
    total = nrow * F1 * F1
    out = torch.full((total + 256,), CANARY, dtype=torch.int32, device="cuda")
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=nrow, ncol=x.shape[1], missing=missing)
    b.predict_interactions_device(d, out.data_ptr(), approximate=approximate, ntree_limit=ntree_limit)
    torch.cuda.synchronize()
    d.free()
    o = out.cpu().numpy().view(np.uint32)
    assert np.all(o[total:] == CANARY), "the device form wrote past nrow * (F + 1)^2"
    return o[:total].view(np.float32).reshape(nrow, F1, F1)


def same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = int(np.sum(helpers.bits(a) != helpers.bits(b)))
    assert diff == 0, (what, diff)


def every_form(torch, b, x, missing, approximate=False, ntree_limit=0):
    """Host and device form, split auto and off: the same bits, returned once."""
    got = []
    for split in ("auto", "off"):
        b.set_param("ohx_contribs_split", split)
        got.append(b.predict_interactions(capi.DMatrix(x, missing=missing), approximate=approximate,
                                          ntree_limit=ntree_limit))
        got.append(device_form(torch, b, x, missing, approximate, ntree_limit))
    b.set_param("ohx_contribs_split", "auto")
    for g, what in zip(got[1:], ("device form", "split off", "split off, device form")):
        same(got[0], g, what)
    return got[0]


def check_identities(b, x, missing, got, ntree_limit=0, rel=1e-5):
    """phi (from predict_contribs) as row sums, the diagonal bit for bit in 1.6.0's order over phi, symmetry, local
    accuracy against the margin, the bias row and column."""
    phi = b.predict_contribs(capi.DMatrix(x, missing=missing), ntree_limit=ntree_limit)
    F = phi.shape[1] - 1
    g = got.astype(np.float64)
    scale = 1.0 + np.abs(g).sum(axis=(1, 2))
    assert np.all(np.abs(g.sum(axis=2) - phi) <= rel * scale[:, None])
    same(np.ascontiguousarray(np.diagonal(got, axis1=1, axis2=2)), isup.diagonal_f32(got, phi), "diagonal")
    assert np.all(np.abs(g - g.transpose(0, 2, 1)) <= rel * scale[:, None, None])
    assert np.all(got[:, F, :F] == 0) and np.all(got[:, :F, F] == 0)
    margin = b.predict(capi.DMatrix(x, missing=missing), option_mask=1, ntree_limit=ntree_limit)
    assert np.all(np.abs(g.sum(axis=(1, 2)) - margin) <= rel * scale)


@pytest.mark.parametrize("ntree,nfeat,depth,p_leaf", cs.CASES)
def test_exact_against_brute_force(torch_cuda, ntree, nfeat, depth, p_leaf):
    rng = np.random.default_rng(9300 + ntree * 100 + nfeat)
    js, trees, base = cs.random_booster(rng, ntree, nfeat, depth, p_leaf)
    rows = cs.random_rows(rng, 16 if nfeat >= 8 else 70, nfeat)
    b = capi.Booster(model_buffer=js)
    for missing in (-999.0, float("nan")):
        ref = isup.brute_force_interactions(trees, base, rows, missing, nfeat)
        got = every_form(torch_cuda, b, rows, missing)
        assert isup.within(got, ref) <= 1.0, missing
        check_identities(b, rows, missing, got)
    if ntree > 2:
        ref = isup.brute_force_interactions(trees, base, rows, -999.0, nfeat, ntree_limit=2)
        got = every_form(torch_cuda, b, rows, -999.0, ntree_limit=2)
        assert isup.within(got, ref) <= 1.0


@pytest.mark.parametrize("which", ["20 trees", "100 trees"])
def test_exact_on_the_oh_recipe(torch_cuda, oh20, deep_model, which):
    """Both launch shapes and forms and the identities on 256 C12 rows of the 20-tree booster and 8 of the 100-tree
    one; against the CPU restatement (2F + 3 TreeSHAP passes a row: about 9 CPU-seconds a row at 20 trees) on 8 and 1
    of them."""
    model = oh20 if which == "20 trees" else deep_model
    n, k = (256, 8) if which == "20 trees" else (8, 1)
    rows = synth.rows_cpu(synth.GRIDS["C12"], 1000, n)
    rng = np.random.default_rng(model.num_trees)
    rows[rng.random(rows.shape) < 2e-3] = np.float32(synth.XX_MISS)
    b = capi.Booster(model_buffer=model.image)
    got = every_form(torch_cuda, b, rows, synth.XX_MISS)
    ref = synth.interactions_cpu(model.image, rows[:k], 27, missing=synth.XX_MISS).astype(np.float64)
    worst = isup.within(got[:k], ref)
    print(f"OH recipe, {which}: worst |got - restated| / (1e-5 (1 + sum |Phi|)) = {worst:.3f}")
    assert worst <= 1.0
    check_identities(b, rows, synth.XX_MISS, got)


@pytest.mark.parametrize("ntree_limit", [0, 7])
def test_approximate_is_contributions_on_the_diagonal(torch_cuda, oh20, ntree_limit):
    rows = synth.rows_cpu(synth.GRIDS["C12"], 5000, 700)
    b = capi.Booster(model_buffer=oh20.image)
    got = every_form(torch_cuda, b, rows, synth.XX_MISS, approximate=True, ntree_limit=ntree_limit)
    phi = b.predict_contribs(capi.DMatrix(rows, missing=synth.XX_MISS), approximate=True, ntree_limit=ntree_limit)
    want = np.zeros_like(got)
    idx = np.arange(28)
    want[:, idx, idx] = phi
    same(got, want, "approximate")


def test_exact_on_long_paths(torch_cuda):
    """Paths of 1 to 32 distinct features (every length class): against float64, bounded by 1.6.0's own float32
    algorithm (the restatement) times 1.5 where 1e-5 cannot hold."""
    rng = np.random.default_rng(43)
    js, trees, base = cs.caterpillar_booster(rng, 10, 40, 32)
    assert synth.contribs_table_stats(js)["max_len"] == 32
    rows = rng.normal(0, 1.0, (96, 40)).astype(np.float32)
    rows[rng.random(rows.shape) < 0.02] = np.nan
    b = capi.Booster(model_buffer=js)
    got = every_form(torch_cuda, b, rows, -999.0)
    ref = isup.interactions64(trees, base, rows, -999.0, 40)
    err = isup.within(got, ref)
    err_r = isup.within(synth.interactions_cpu(js, rows, 40, missing=-999.0), ref)
    print(f"long paths: kernels {err:.3f}, 1.6.0's algorithm in float32 {err_r:.3f} (x 1e-5 (1 + sum |Phi|))")
    assert err <= max(1.0, 1.5 * err_r)
    assert np.all(np.isfinite(got))
    check_identities(b, rows, -999.0, got, rel=1e-3)


@functools.lru_cache(maxsize=None)
def adversarial(ntree, zero):
    js, trees = S.contribs_booster(3000 + ntree + (500 if zero else 0), ntree, zero)
    base = float(np.float32(json.loads(js)["learner"]["learner_model_param"]["base_score"]))
    return js, cs.tree_dicts(trees), base, trees


@pytest.mark.parametrize("ntree,zero", [(2, False), (5, False), (10, False), (5, True)])
def test_adversarial_boosters(torch_cuda, ntree, zero):
    """Repeated features on paths of up to 27 distinct features, leaf covers of 1 against 1000 (and 0), rows on
    thresholds, every missing marker: finite, all forms agree, and no worse than 1.5 times 1.6.0's float32 algorithm
    against float64 (or within 1e-5)."""
    js, d, base, trees = adversarial(ntree, zero)
    b = capi.Booster(model_buffer=js)
    for missing in (-999.0, float("nan"), float("inf"), float("-inf")):
        x = S.rows_for(ntree * 10 + 1, trees, 24, missing)
        got = every_form(torch_cuda, b, x, missing)
        assert np.all(np.isfinite(got))
        ref = isup.interactions64(d, base, x, missing, S.NFEAT)
        err = isup.within(got, ref)
        err_r = isup.within(synth.interactions_cpu(js, x, S.NFEAT, missing=missing), ref)
        print(f"{ntree} trees{' zero covers' if zero else ''}, missing {missing}: kernels {err:.3f}, "
              f"1.6.0's algorithm {err_r:.3f} (x 1e-5 (1 + sum |Phi|))")
        assert err <= max(1.0, 1.5 * err_r), (missing, err, err_r)


@pytest.mark.parametrize("nrow", [0, 1, 63, 64, 65])
def test_row_counts(torch_cuda, nrow):
    rng = np.random.default_rng(51)
    js, trees, base = cs.random_booster(rng, 6, 6, 5, 0.2)
    x = cs.random_rows(rng, max(nrow, 1), 6)[:nrow]
    assert synth.interactions_plan(nrow, 6, 6)[0] == (nrow > 0)
    b = capi.Booster(model_buffer=js)
    got = every_form(torch_cuda, b, x, -999.0) if nrow else None
    dev = device_form(torch_cuda, b, x if nrow else np.zeros((0, 6), np.float32), -999.0, nrow=nrow)
    if nrow:
        assert isup.within(got, isup.brute_force_interactions(trees, base, x, -999.0, 6)) <= 1.0
    else:
        assert dev.shape == (0, 7, 7)
        assert b.predict_interactions(capi.DMatrix(np.zeros((0, 6), np.float32), missing=-999.0)).shape[0] == 0


def test_fewer_columns_than_features(torch_cuda):
    rng = np.random.default_rng(52)
    js, trees, base = cs.random_booster(rng, 5, 7, 5, 0.2)
    x = np.ascontiguousarray(cs.random_rows(rng, 70, 7)[:, :4])
    b = capi.Booster(model_buffer=js)
    got = every_form(torch_cuda, b, x, -999.0)
    assert isup.within(got, isup.brute_force_interactions(trees, base, x, -999.0, 7)) <= 1.0


@pytest.mark.parametrize("nfeat", [1, 128])
def test_feature_counts(torch_cuda, nfeat):
    rng = np.random.default_rng(53 + nfeat)
    js, trees, base = cs.random_booster(rng, 12, nfeat, 4, 0.1)
    x = cs.random_rows(rng, 70, nfeat)
    b = capi.Booster(model_buffer=js)
    assert synth.interactions_plan(70, nfeat, 12)[0]
    got = every_form(torch_cuda, b, x, -999.0)
    ref = isup.interactions64(trees, base, x, -999.0, nfeat)
    assert isup.within(got, ref) <= 1.0
    if nfeat == 1:
        assert np.all(got[:, 0, 0] == b.predict_contribs(capi.DMatrix(x, missing=-999.0))[:, 0])


@pytest.mark.parametrize("ntree_limit", [1, 50])
def test_ntree_limit(torch_cuda, ntree_limit):
    rng = np.random.default_rng(54)
    js, trees, base = cs.random_booster(rng, 7, 6, 5, 0.2)
    x = cs.random_rows(rng, 100, 6)
    b = capi.Booster(model_buffer=js)
    assert synth.interactions_plan(100, 6, min(ntree_limit, 7))[0] == (ntree_limit > 1)
    got = every_form(torch_cuda, b, x, -999.0, ntree_limit=ntree_limit)
    ref = isup.brute_force_interactions(trees, base, x, -999.0, 6, ntree_limit=min(ntree_limit, 7))
    assert isup.within(got, ref) <= 1.0
    for ap in (False, True):
        assert np.array_equal(helpers.bits(b.predict_interactions(capi.DMatrix(x, missing=-999.0), approximate=ap,
                                                                  ntree_limit=ntree_limit)),
                              helpers.bits(b.predict_interactions(capi.DMatrix(x, missing=-999.0), approximate=ap,
                                                                  ntree_limit=0 if ntree_limit > 7 else ntree_limit)))


def test_split_direct_switch_and_part_budget(torch_cuda):
    """4 096 direct waves (tiles x features) still split, one tile more does not; and a batch whose `part` would pass
    1 GiB goes direct.  The bits are the same either side."""
    rng = np.random.default_rng(55)
    js, _, _ = cs.random_booster(rng, 4, 32, 4, 0.1)
    b = capi.Booster(model_buffer=js)
    x = cs.random_rows(rng, 64 * 129, 32)
    assert synth.interactions_plan(64 * 128, 32, 4)[0] and not synth.interactions_plan(64 * 129, 32, 4)[0]
    whole = b.predict_interactions(capi.DMatrix(x, missing=-999.0))
    head = b.predict_interactions(capi.DMatrix(np.ascontiguousarray(x[:64 * 128]), missing=-999.0))
    same(head, whole[:64 * 128], "split / direct")
    # part: 1 tile x 128 features x 257 trees x 128 x 64 floats > 1 GiB
    js2, _, _ = cs.random_booster(rng, 257, 128, 1, 0.0)
    b2 = capi.Booster(model_buffer=js2)
    x2 = cs.random_rows(rng, 64, 128)
    assert not synth.interactions_plan(64, 128, 257)[0] and synth.interactions_plan(64, 128, 256)[0]
    a257 = b2.predict_interactions(capi.DMatrix(x2, missing=-999.0))
    a256 = b2.predict_interactions(capi.DMatrix(x2, missing=-999.0), ntree_limit=256)
    b2.set_param("ohx_contribs_split", "off")
    same(a256, b2.predict_interactions(capi.DMatrix(x2, missing=-999.0), ntree_limit=256), "256 trees split / off")
    same(a257, b2.predict_interactions(capi.DMatrix(x2, missing=-999.0)), "257 trees direct")


def test_direct_launches_past_8192_waves(torch_cuda):
    """128 features: a direct launch holds 64 tiles; 65 tiles take two, the second starting at tile 64.  Rows of the
    second launch match the same rows predicted on their own."""
    rng = np.random.default_rng(58)
    js, _, _ = cs.random_booster(rng, 3, 128, 3, 0.1)
    b = capi.Booster(model_buffer=js)
    x = cs.random_rows(rng, 64 * 65, 128)
    b.set_param("ohx_contribs_split", "off")
    assert synth.interactions_plan(len(x), 128, 3, allow_split=False)[3] == 2
    whole = b.predict_interactions(capi.DMatrix(x, missing=-999.0))
    tail = b.predict_interactions(capi.DMatrix(np.ascontiguousarray(x[64 * 64:]), missing=-999.0))
    same(whole[64 * 64:], tail, "second direct launch")
    same(whole[:64], b.predict_interactions(capi.DMatrix(np.ascontiguousarray(x[:64]), missing=-999.0)), "first")


def test_deterministic_across_calls_batches_and_forms(torch_cuda):
    rng = np.random.default_rng(56)
    js, _, _ = cs.random_booster(rng, 9, 8, 6, 0.15)
    big = cs.random_rows(rng, 300, 8)
    b = capi.Booster(model_buffer=js)
    whole = b.predict_interactions(capi.DMatrix(big, missing=-999.0))
    same(whole, b.predict_interactions(capi.DMatrix(big, missing=-999.0)), "second call")
    for r in (0, 77, 299):
        alone = b.predict_interactions(capi.DMatrix(np.ascontiguousarray(big[r:r + 1]), missing=-999.0))
        same(alone[0], whole[r], f"row {r} alone")
        same(device_form(torch_cuda, b, np.ascontiguousarray(big[r:r + 1]), -999.0)[0], whole[r], f"row {r} device")


def test_refusals(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(57)
    js, _, _ = cs.random_booster(rng, 3, 4, 4, 0.1)
    rows = cs.random_rows(rng, 64, 4)
    d = capi.DMatrix(rows, missing=-999.0)
    with pytest.raises(capi.OhxError, match="no model"):
        capi.Booster().predict_interactions(d)
    doc = json.loads(js)
    for t in doc["learner"]["gradient_booster"]["model"]["trees"]:
        t["sum_hessian"] = [0.0] * len(t["sum_hessian"])
    with pytest.raises(capi.OhxError, match="no cover statistics"):
        capi.Booster(model_buffer=json.dumps(doc).encode()).predict_interactions(d)
    b = capi.Booster(model_buffer=js)
    with pytest.raises(capi.OhxError, match="Number of columns does not match"):
        b.predict_interactions(capi.DMatrix(cs.random_rows(rng, 64, 6), missing=-999.0))
    with pytest.raises(capi.OhxError, match="d_out is NULL"):
        b.predict_interactions_device(d, 0)
    with pytest.raises(capi.OhxError, match="at most 128"):
        capi.Booster(model_buffer=cs.random_booster(rng, 2, 129, 2, 0.0)[0]).predict_interactions(
            capi.DMatrix(cs.random_rows(rng, 4, 129), missing=-999.0))
    js33, _, _ = cs.caterpillar_booster(rng, 2, 40, 33)
    with pytest.raises(capi.OhxError, match="at most 32"):
        capi.Booster(model_buffer=js33).predict_interactions(capi.DMatrix(cs.random_rows(rng, 4, 40), missing=-999.0))
    # +-inf in a column no tree splits on (feature 3 of a 5-feature booster that only splits on 0 - 2)
    js5, _, _ = cs.random_booster(rng, 3, 3, 3, 0.1)
    doc5 = json.loads(js5)
    doc5["learner"]["learner_model_param"]["num_feature"] = "5"
    b5 = capi.Booster(model_buffer=json.dumps(doc5).encode())
    x5 = cs.random_rows(rng, 70, 5)
    for ap in (False, True):
        for v in (np.inf, -np.inf):
            xi = x5.copy()
            xi[40, 3] = v
            with pytest.raises(capi.OhxError, match="inf"):
                b5.predict_interactions(capi.DMatrix(xi, missing=-999.0), approximate=ap)
        assert b5.predict_interactions(capi.DMatrix(x5, missing=-999.0), approximate=ap).shape == (70, 6, 6)
    # a capture is refused, and the booster and the stream stay usable
    out = torch.zeros((64, 5, 5), dtype=torch.float32, device="cuda")
    t = torch.from_numpy(rows).cuda()
    dd = capi.DMatrix(device_ptr=t.data_ptr(), nrow=64, ncol=4, missing=-999.0)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="not capturable"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.predict_interactions_device(dd, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        b.predict_interactions_device(dd, out.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    same(out.cpu().numpy(), b.predict_interactions(d), "after the refused capture")
    # an output that cannot be allocated: refused with a message, nothing launched (the rows are never read)
    huge = capi.DMatrix(device_ptr=t.data_ptr(), nrow=1 << 40, ncol=4, missing=-999.0)
    with pytest.raises(capi.OhxError):
        b.predict_interactions(huge)
    same(out.cpu().numpy(), b.predict_interactions(d), "after the failed allocation")


def test_the_booster_moved_to_another_device(torch_cuda, oh20):
    torch = torch_cuda
    rows = synth.rows_cpu(synth.GRIDS["C12"], 3000, 100)
    b = capi.Booster(model_buffer=oh20.image)
    want = {ap: b.predict_interactions(capi.DMatrix(rows, missing=synth.XX_MISS), approximate=ap)
            for ap in (False, True)}
    target = 1 if torch.cuda.device_count() >= 2 else 0
    b.set_param("ohx_device", str(target))
    torch.cuda.set_device(target)
    try:
        for ap in (True, False):
            same(b.predict_interactions(capi.DMatrix(rows, missing=synth.XX_MISS), approximate=ap), want[ap], ap)
    finally:
        torch.cuda.set_device(0)


def test_buffers_stay_apart_from_a_captured_predict(torch_cuda, deep_model):
    torch = torch_cuda
    grid = (12, 72, 72)
    nrow = 12 * 72 * 40
    rows_np = synth.rows_cpu(grid, 0, nrow)
    rows = torch.from_numpy(rows_np).cuda()
    out = torch.zeros(nrow, dtype=torch.float32, device="cuda")
    b = capi.Booster(model_buffer=deep_model.image)
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=nrow, ncol=27, missing=synth.XX_MISS)
    d.set_grid(grid[0], grid[1], 0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.predict_device(d, out.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.predict_device(d, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    bigger = synth.rows_cpu(synth.GRIDS["C48"], 0, 2 * nrow)
    c = b.predict_interactions(capi.DMatrix(bigger, missing=synth.XX_MISS), approximate=True)
    assert c.shape == (2 * nrow, 28, 28)
    c = b.predict_interactions(capi.DMatrix(bigger[:64], missing=synth.XX_MISS))
    assert c.shape == (64, 28, 28)
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    b.check()
    want = helpers.oracle_predict(deep_model.image, rows_np, synth.XX_MISS)
    same(out.cpu().numpy(), want, "replay")
