"""Per-feature contributions on the GPU (OHXBoosterPredictContribs / ...Device, csrc/contribs.hip): exact TreeSHAP
against the float64 brute force and the CPU restatement, approximate mode bit for bit against the restatement, local
accuracy against the margin, determinism across calls, forms and launch shapes, the refusals, and buffers kept apart
from a captured predict's."""
import json

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import contribs_support as cs
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def contribs_model():
    """The synthetic OH recipe at 20 trees (depth <= 18, grown on C12)."""
    return synth.make_model(num_trees=20, max_depth=18, sample_log2=16, min_leaf=2, grid=synth.GRIDS["C12"])


def _device_contribs(torch, b, rows, missing, nfeat, approximate=False, ntree_limit=0):
    t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    out = torch.full((len(rows), nfeat + 1), float("nan"), dtype=torch.float32, device="cuda")
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=len(rows), ncol=rows.shape[1], missing=missing)
    b.predict_contribs_device(d, out.data_ptr(), approximate=approximate, ntree_limit=ntree_limit)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    d.free()
    return res


def _salted(rows, seed, rate=2e-3):
    rows = rows.copy()
    rng = np.random.default_rng(seed)
    mask = rng.random(rows.shape) < rate
    rows[mask] = np.where(rng.random(int(mask.sum())) < 0.5, np.float32(synth.XX_MISS), np.float32(np.nan))
    return rows


@pytest.mark.parametrize("ntree,nfeat,depth,p_leaf", cs.CASES)
def test_exact_against_brute_force(torch_cuda, ntree, nfeat, depth, p_leaf):
    rng = np.random.default_rng(7000 + ntree * 100 + nfeat)
    js, trees, base = cs.random_booster(rng, ntree, nfeat, depth, p_leaf)
    rows = cs.random_rows(rng, 40 if nfeat >= 8 else 120, nfeat)
    b = capi.Booster(model_buffer=js)
    for missing in (-999.0, float("nan")):
        ref = cs.brute_force(trees, base, rows, missing, nfeat)
        host = b.predict_contribs(capi.DMatrix(rows, missing=missing))
        dev = _device_contribs(torch_cuda, b, rows, missing, nfeat)
        assert cs.within(host, ref) <= 1.0, missing
        assert np.array_equal(helpers.bits(host), helpers.bits(dev))
    if nfeat > 2:
        part = np.ascontiguousarray(rows[:, :nfeat - 2])
        got = b.predict_contribs(capi.DMatrix(part, missing=-999.0))
        assert cs.within(got, cs.brute_force(trees, base, part, -999.0, nfeat)) <= 1.0


@pytest.mark.parametrize("which", ["20 trees", "100 trees"])
def test_exact_on_the_oh_recipe(contribs_model, deep_model, which):
    """Both launch shapes - trees split over waves (the default for a batch this small) and one wave per 64 rows over
    every tree ("ohx_contribs_split" = off) - against the CPU restatement, and against each other bit for bit."""
    model = contribs_model if which == "20 trees" else deep_model
    rows = _salted(synth.rows_cpu(synth.GRIDS["C12"], 1000, 256), seed=model.num_trees)
    ref = synth.contribs_cpu(model.image, rows, 27, missing=synth.XX_MISS).astype(np.float64)
    b = capi.Booster(model_buffer=model.image)
    split = b.predict_contribs(capi.DMatrix(rows, missing=synth.XX_MISS))
    b.set_param("ohx_contribs_split", "off")
    direct = b.predict_contribs(capi.DMatrix(rows, missing=synth.XX_MISS))
    worst = cs.within(split, ref)
    assert worst <= 1.0, f"worst |got - ref| / bound = {worst:.3f} ({which})"
    assert np.array_equal(helpers.bits(split), helpers.bits(direct))


def test_exact_on_long_paths(torch_cuda):
    """Paths of every length from 1 to 32 distinct features: every length class of the exact kernels, both launch
    shapes, against the CPU restatement and local accuracy against the margin."""
    rng = np.random.default_rng(41)
    js, trees, base = cs.caterpillar_booster(rng, 24, 40, 32)
    assert synth.contribs_table_stats(js)["max_len"] == 32
    rows = rng.normal(0, 1.0, (1000, 40)).astype(np.float32)
    rows[rng.random(rows.shape) < 0.02] = np.nan
    # the reference is float64 TreeSHAP: on 32-feature paths float32 rounding in the recurrences alone - 1.6.0's own
    # recursive algorithm included (test_contribs_cpu.py::test_float32_error_grows_with_path_length, 2.2x) - exceeds
    # 1e-5 * (1 + sum |phi|); the bound here is 1e-4 (docs/12_contributions.md section 12.4 gives the measurements)
    ref = cs.treeshap64(trees, base, rows, -999.0, 40)
    b = capi.Booster(model_buffer=js)
    got = b.predict_contribs(capi.DMatrix(rows, missing=-999.0))
    worst = cs.within(got, ref)
    print(f"long paths: worst |got - ref64| / (1e-5 (1 + sum |ref|)) = {worst:.3f}")
    assert worst <= 10.0
    g = got.astype(np.float64)
    acc = np.abs(g.sum(axis=1) - helpers.oracle_predict(synth.convert_model(js, "binary"), rows, -999.0, option_mask=1))
    print(f"long paths: worst local accuracy / (1 + sum |phi|) = {np.max(acc / (1.0 + np.abs(g).sum(axis=1))):.3g}")
    b.set_param("ohx_contribs_split", "off")
    assert np.array_equal(helpers.bits(got), helpers.bits(b.predict_contribs(capi.DMatrix(rows, missing=-999.0))))
    margin = helpers.oracle_predict(synth.convert_model(js, "binary"), rows, -999.0, option_mask=1)
    g = got.astype(np.float64)
    # local accuracy adds the 40 columns' rounding up: 1.6.0's float32 algorithm itself is off by up to 1.7e-4 * (1 +
    # sum |phi|) here, against 4e-7 for the float64 reference
    assert np.all(np.abs(g.sum(axis=1) - margin) <= 1e-3 * (1.0 + np.abs(g).sum(axis=1)))
    # over 32 distinct features on one path: exact mode is refused, approximate mode is not
    js33, _, _ = cs.caterpillar_booster(rng, 2, 40, 33)
    b33 = capi.Booster(model_buffer=js33)
    with pytest.raises(capi.OhxError, match="at most 32"):
        b33.predict_contribs(capi.DMatrix(rows, missing=-999.0))
    assert b33.predict_contribs(capi.DMatrix(rows, missing=-999.0), approximate=True).shape == (1000, 41)


def test_the_booster_moved_to_another_device(torch_cuda, contribs_model):
    """"ohx_device" between two contribs calls: the booster's device state is dropped and the next call builds the
    tables again where the booster now is, and takes that device's stream - same bits.  On one GPU the move is to the
    device it is on (the device state is dropped all the same); with two, to the second."""
    torch = torch_cuda
    rows = _salted(synth.rows_cpu(synth.GRIDS["C12"], 3000, 700), seed=5)
    b = capi.Booster(model_buffer=contribs_model.image)
    want = {ap: b.predict_contribs(capi.DMatrix(rows, missing=synth.XX_MISS), approximate=ap) for ap in (False, True)}
    target = 1 if torch.cuda.device_count() >= 2 else 0
    b.set_param("ohx_device", str(target))
    torch.cuda.set_device(target)
    try:
        d = capi.DMatrix(rows, missing=synth.XX_MISS)
        for ap in (True, False):
            assert np.array_equal(helpers.bits(b.predict_contribs(d, approximate=ap)), helpers.bits(want[ap]))
        t = torch.from_numpy(rows).cuda(target)
        out = torch.zeros((len(rows), 28), dtype=torch.float32, device=f"cuda:{target}")
        dd = capi.DMatrix(device_ptr=t.data_ptr(), nrow=len(rows), ncol=27, missing=synth.XX_MISS)
        b.predict_contribs_device(dd, out.data_ptr(), stream=torch.cuda.current_stream(target).cuda_stream)
        torch.cuda.synchronize(target)
        assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(want[False]))
    finally:
        torch.cuda.set_device(0)


@pytest.mark.parametrize("ntree_limit", [0, 9])
def test_approximate_is_bit_exact(contribs_model, ntree_limit):
    rows = _salted(synth.rows_cpu(synth.GRIDS["C12"], 5000, 3000), seed=3)
    b = capi.Booster(model_buffer=contribs_model.image)
    got = b.predict_contribs(capi.DMatrix(rows, missing=synth.XX_MISS), approximate=True, ntree_limit=ntree_limit)
    ref = synth.contribs_cpu(contribs_model.image, rows, 27, missing=synth.XX_MISS, approximate=True,
                             ntree_limit=ntree_limit)
    assert np.array_equal(helpers.bits(got), helpers.bits(ref))


@pytest.mark.parametrize("approximate", [False, True])
@pytest.mark.parametrize("ntree_limit", [0, 5])
def test_local_accuracy_against_the_margin(torch_cuda, contribs_model, approximate, ntree_limit):
    torch = torch_cuda
    rows = _salted(synth.rows_cpu(synth.GRIDS["C12"], 20000, 2000), seed=4)
    b = capi.Booster(model_buffer=contribs_model.image)
    t = torch.from_numpy(rows).cuda()
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=len(rows), ncol=27, missing=synth.XX_MISS)
    margin = torch.zeros(len(rows), dtype=torch.float32, device="cuda")
    b.predict_device(d, margin.data_ptr(), option_mask=1, ntree_limit=ntree_limit)
    torch.cuda.synchronize()
    got = b.predict_contribs(d, approximate=approximate, ntree_limit=ntree_limit).astype(np.float64)
    m = margin.cpu().numpy().astype(np.float64)
    scale = 1.0 + np.abs(got).sum(axis=1)
    assert np.all(np.abs(got.sum(axis=1) - m) <= 1e-5 * scale)


@pytest.mark.parametrize("approximate", [False, True])
def test_deterministic_across_calls_forms_and_batches(torch_cuda, approximate):
    """Two calls, host and device forms, and the first 4 096 rows alone (trees split over waves, a second launch) or
    inside a 300 000-row batch (one wave per tile walks every tree): the same bits."""
    torch = torch_cuda
    rng = np.random.default_rng(21)
    js, _, _ = cs.random_booster(rng, 12, 10, 9, 0.15)
    big = cs.random_rows(rng, 300_000, 10)
    b = capi.Booster(model_buffer=js)
    small = np.ascontiguousarray(big[:4096])
    a1 = b.predict_contribs(capi.DMatrix(small, missing=-999.0), approximate=approximate)
    a2 = b.predict_contribs(capi.DMatrix(small, missing=-999.0), approximate=approximate)
    dev = _device_contribs(torch, b, small, -999.0, 10, approximate=approximate)
    whole = b.predict_contribs(capi.DMatrix(big, missing=-999.0), approximate=approximate)
    for other in (a2, dev, whole[:4096]):
        assert np.array_equal(helpers.bits(a1), helpers.bits(other))


def test_refusals(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(31)
    js, _, _ = cs.random_booster(rng, 3, 4, 4, 0.1)
    rows = cs.random_rows(rng, 64, 4)
    d = capi.DMatrix(rows, missing=-999.0)
    empty = capi.Booster()
    with pytest.raises(capi.OhxError, match="no model"):
        empty.predict_contribs(d)
    doc = json.loads(js)
    for t in doc["learner"]["gradient_booster"]["model"]["trees"]:
        t["sum_hessian"] = [0.0] * len(t["sum_hessian"])
    with pytest.raises(capi.OhxError, match="no cover statistics"):
        capi.Booster(model_buffer=json.dumps(doc).encode()).predict_contribs(d)
    b = capi.Booster(model_buffer=js)
    wide = cs.random_rows(rng, 64, 6)
    with pytest.raises(capi.OhxError, match="Number of columns does not match"):
        b.predict_contribs(capi.DMatrix(wide, missing=-999.0))
    with pytest.raises(capi.OhxError, match="d_out is NULL"):
        b.predict_contribs_device(d, 0)
    out = torch.zeros((64, 5), dtype=torch.float32, device="cuda")
    t = torch.from_numpy(rows).cuda()
    dd = capi.DMatrix(device_ptr=t.data_ptr(), nrow=64, ncol=4, missing=-999.0)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="not capturable"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.predict_contribs_device(dd, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    # the booster is still usable, and so is the stream
    with torch.cuda.stream(s):
        b.predict_contribs_device(dd, out.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(b.predict_contribs(d)))


@pytest.mark.parametrize("approximate", [False, True])
def test_a_failed_allocation_leaves_no_error_behind(torch_cuda, approximate):
    """An output that cannot be allocated (2**40 borrowed rows) is refused with a message before anything is launched,
    and the failure is forgotten with it: the next host call and the next device call on the caller's stream give the
    bits of the call before."""
    torch = torch_cuda
    rng = np.random.default_rng(33)
    js, _, _ = cs.random_booster(rng, 3, 4, 4, 0.1)
    rows = cs.random_rows(rng, 64, 4)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(rows, missing=-999.0)
    before = b.predict_contribs(d, approximate=approximate)
    t = torch.from_numpy(rows).cuda()
    huge = capi.DMatrix(device_ptr=t.data_ptr(), nrow=1 << 40, ncol=4, missing=-999.0)
    with pytest.raises(capi.OhxError):
        b.predict_contribs(huge, approximate=approximate)
    assert np.array_equal(helpers.bits(b.predict_contribs(d, approximate=approximate)), helpers.bits(before))
    out = torch.zeros((64, 5), dtype=torch.float32, device="cuda")
    dd = capi.DMatrix(device_ptr=t.data_ptr(), nrow=64, ncol=4, missing=-999.0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.predict_contribs_device(dd, out.data_ptr(), approximate=approximate, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(before))


def test_buffers_stay_apart_from_a_captured_predict(torch_cuda, deep_model):
    """A predict captured into a hipGraph holds raw pointers to the booster's buffers: a contribs call on a bigger batch
    in between must not move them - the replay still matches the oracle bit for bit."""
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
    c = b.predict_contribs(capi.DMatrix(bigger, missing=synth.XX_MISS), approximate=True)
    assert c.shape == (2 * nrow, 28)
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    b.check()
    want = helpers.oracle_predict(deep_model.image, rows_np, synth.XX_MISS)
    assert np.array_equal(helpers.bits(out.cpu().numpy()), helpers.bits(want))
