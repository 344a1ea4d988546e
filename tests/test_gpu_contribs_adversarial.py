"""Feature contributions on the GPU (csrc/contribs.hip) on adversarial boosters and at the edges of their launch
shapes.

The boosters (tests/booster_shapes.py contribs_booster) hold chains of up to 27 distinct features that split on some
feature again (the 24- and 32-feature length classes of the exact kernels, with merged path elements), 1 / 1000 leaf
covers, thresholds on +-0, denormals and +-3e38, and rows half of which sit on a threshold or one float32 step from it.
Every case runs through both launch shapes ("ohx_contribs_split" auto and off) and both matrix forms (host and
device): all four agree bit for bit.  The launch-shape cases first ask synth.contribs_plan which shape the library
takes, so that none can pass on another shape than the one it is named for."""
import functools
import json

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import contribs_support as cs
from tests import helpers

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 5, 10, 135)
MISSING = (-999.0, float("nan"), float("inf"), float("-inf"))
CANARY = 0x7FC0DEAD           # a NaN whose bits the kernels never produce: what the device form must leave alone
TILE = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@functools.lru_cache(maxsize=None)
def booster(ntree, zero_cover_leaves=False):
    js, trees = S.contribs_booster(3000 + ntree + (500 if zero_cover_leaves else 0), ntree, zero_cover_leaves)
    base = float(np.float32(json.loads(js)["learner"]["learner_model_param"]["base_score"]))
    return js, trees, base, cs.tree_dicts(trees), synth.contribs_table_stats(js)["max_len"]


@functools.lru_cache(maxsize=None)
def rows(ntree, missing, n=512):
    return S.rows_for(ntree * 10 + 1, booster(ntree)[1], n, missing)


def same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = int(np.sum(helpers.bits(a) != helpers.bits(b)))
    assert diff == 0, (what, diff)


def device_form(torch, b, x, missing, approximate=False, ntree_limit=0, nrow=None):
    """The device form into a buffer with a canary behind the nrow * (F + 1) floats it may write: the canary must
    survive, and with 0 rows the whole buffer."""
    nrow = len(x) if nrow is None else nrow
    F = b.info()["num_feature"]
    t = torch.from_numpy(np.ascontiguousarray(x if len(x) else np.zeros((1, x.shape[1]), np.float32))).cuda()
    total = nrow * (F + 1)
    out = torch.full((total + 256,), CANARY, dtype=torch.int32, device="cuda")
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=nrow, ncol=x.shape[1], missing=missing)
    b.predict_contribs_device(d, out.data_ptr(), approximate=approximate, ntree_limit=ntree_limit)
    torch.cuda.synchronize()
    d.free()
    o = out.cpu().numpy().view(np.uint32)
    assert np.all(o[total:] == CANARY), "the device form wrote past nrow * (F + 1)"
    return o[:total].view(np.float32).reshape(nrow, F + 1)


def every_form(torch, b, x, missing, approximate=False, ntree_limit=0):
    """Host and device form, split auto and off: the same bits, returned once."""
    got = []
    for split in ("auto", "off"):
        b.set_param("ohx_contribs_split", split)
        got.append(b.predict_contribs(capi.DMatrix(x, missing=missing), approximate=approximate,
                                      ntree_limit=ntree_limit))
        got.append(device_form(torch, b, x, missing, approximate, ntree_limit))
    b.set_param("ohx_contribs_split", "auto")
    for g, what in zip(got[1:], ("device form", "split off", "split off, device form")):
        same(got[0], g, what)
    return got[0]


def bound_exact(got, ref64, restated, max_len, what):
    """1e-5 (1 + sum |phi|) against float64 TreeSHAP; where paths exceed 18 distinct features, float32 cannot hold that
    (docs/12_contributions.md 12.4): no worse than 1.5 times xgboost 1.6.0's own algorithm in float32 (the CPU
    restatement) on the same rows, and within the 1e-4 the caterpillar test allows."""
    err = cs.within(got, ref64)
    err_r = cs.within(restated, ref64)
    print(f"{what}: kernels {err:.3f}, 1.6.0's algorithm in float32 {err_r:.3f} (x 1e-5 (1 + sum |phi|))")
    if max_len <= 18:
        assert err <= 1.0, (what, err)
    else:
        assert err <= max(1.0, 1.5 * err_r) and err <= 10.0, (what, err, err_r)


def local_accuracy(got, image, x, missing, max_len, what, ntree_limit=0):
    margin = helpers.oracle_predict(synth.convert_model(image, "binary"), x, missing, option_mask=1,
                                    ntree_limit=ntree_limit)
    g = got.astype(np.float64)
    worst = float(np.max(np.abs(g.sum(axis=1) - margin) / (1.0 + np.abs(g).sum(axis=1)))) if len(g) else 0.0
    print(f"{what}: local accuracy {worst:.3g} (1 + sum |phi|)")
    assert worst <= (1e-5 if max_len <= 18 else 1e-3), (what, worst)


def test_the_boosters_reach_the_long_length_classes():
    """The set reaches the 24- and 32-feature length classes with a repeated feature on such a path."""
    classes = set()
    for n in COUNTS:
        trees = booster(n)[1]
        for d, rep in (x for t in trees for x in S.distinct_path_lengths(t)):
            if rep and 21 <= d <= 24:
                classes.add(24)
            if rep and 25 <= d <= 27:
                classes.add(32)
    assert classes == {24, 32}
    assert max(booster(n)[4] for n in COUNTS) == 27


@pytest.mark.parametrize("ntree", COUNTS)
def test_exact_on_adversarial_boosters(torch_cuda, ntree):
    js, trees, base, d, max_len = booster(ntree)
    b = capi.Booster(model_buffer=js)
    for missing in MISSING:
        x = rows(ntree, missing)
        got = every_form(torch_cuda, b, x, missing)
        restated = synth.contribs_cpu(js, x, S.NFEAT, missing=missing)
        # float64 TreeSHAP on every row up to 10 trees; on 135, on 32 random rows and 32 tie rows
        pick = np.arange(len(x)) if ntree <= 10 else np.r_[0:32, len(x) - 32:len(x)]
        ref64 = cs.treeshap64(d, base, x[pick], missing, S.NFEAT)
        bound_exact(got[pick], ref64, restated[pick], max_len, f"{ntree} trees, missing {missing}")
        if max_len <= 18:
            assert cs.within(got, restated.astype(np.float64)) <= 1.0
        local_accuracy(got, js, x, missing, max_len, f"{ntree} trees, missing {missing}")


@pytest.mark.parametrize("ntree", COUNTS)
def test_approximate_on_adversarial_boosters(torch_cuda, ntree):
    js, trees, base, d, _ = booster(ntree)
    b = capi.Booster(model_buffer=js)
    for missing in MISSING:
        x = rows(ntree, missing)
        got = every_form(torch_cuda, b, x, missing, approximate=True)
        same(got, synth.contribs_cpu(js, x, S.NFEAT, missing=missing, approximate=True), f"restatement {missing}")
        k = len(x) if ntree <= 10 else 128
        assert cs.within(got[:k], cs.saabas64(d, base, x[:k], missing, S.NFEAT)) <= 1.0, missing


def test_zero_cover_leaves(torch_cuda):
    """Leaves of cover 0 give zero fractions of exactly 0 (the exact kernel's zinv = 0 branch): finite in both modes,
    the Shapley value on 8 features (brute force) and float64 TreeSHAP on the adversarial shapes."""
    torch = torch_cuda
    rng = np.random.default_rng(17)
    js, trees, base = cs.random_booster(rng, 6, 8, 7, 0.2, zero_leaves=0.3)
    x = cs.random_rows(rng, 200, 8)
    b = capi.Booster(model_buffer=js)
    for missing in (-999.0, float("nan")):
        got = every_form(torch, b, x, missing)
        assert np.all(np.isfinite(got))
        assert cs.within(got, cs.brute_force(trees, base, x, missing, 8)) <= 1.0, missing
        ap = every_form(torch, b, x, missing, approximate=True)
        same(ap, synth.contribs_cpu(js, x, 8, missing=missing, approximate=True), "approximate")
        assert cs.within(ap, cs.saabas64(trees, base, x, missing, 8)) <= 1.0
    js, trees, base, d, max_len = booster(10, zero_cover_leaves=True)
    b = capi.Booster(model_buffer=js)
    x = S.rows_for(77, trees, 512, -999.0)
    got = every_form(torch, b, x, -999.0)
    assert np.all(np.isfinite(got))
    bound_exact(got, cs.treeshap64(d, base, x, -999.0, S.NFEAT), synth.contribs_cpu(js, x, S.NFEAT, missing=-999.0),
                max_len, "zero-cover leaves")
    ap = every_form(torch, b, x, -999.0, approximate=True)
    same(ap, synth.contribs_cpu(js, x, S.NFEAT, missing=-999.0, approximate=True), "approximate, zero covers")


@pytest.mark.parametrize("nrow", [0, 1, 63, 64, 65])
def test_row_counts(torch_cuda, nrow):
    """Partial last tiles and an empty batch, both shapes and forms: the device form writes exactly nrow * (F + 1)
    floats (nothing with 0 rows)."""
    js, trees, base, d, max_len = booster(10)
    b = capi.Booster(model_buffer=js)
    x = np.ascontiguousarray(rows(10, float("nan"))[-nrow:] if nrow else np.zeros((0, S.NFEAT), np.float32))
    for approximate in (False, True):
        if nrow == 0:
            for split in ("auto", "off"):
                b.set_param("ohx_contribs_split", split)
                assert b.predict_contribs(capi.DMatrix(x, missing=np.nan), approximate=approximate).size == 0
                assert device_form(torch_cuda, b, x, np.nan, approximate).shape == (0, S.NFEAT + 1)
            continue
        got = every_form(torch_cuda, b, x, np.nan, approximate)
        same(got, every_form(torch_cuda, b, rows(10, float("nan")), np.nan, approximate)[-nrow:], "inside 512 rows")
        if approximate:
            same(got, synth.contribs_cpu(js, x, S.NFEAT, missing=np.nan, approximate=True), "restatement")


@pytest.mark.parametrize("approximate", [False, True])
def test_ntree_limit(torch_cuda, approximate):
    js, trees, base, d, max_len = booster(10)
    b = capi.Booster(model_buffer=js)
    x = rows(10, -999.0)
    for limit in (1, 2, 5, 10 + 7):
        assert synth.contribs_plan(len(x), S.NFEAT, min(limit, 10))[0] == (limit >= 2)
        got = every_form(torch_cuda, b, x, -999.0, approximate, limit)
        restated = synth.contribs_cpu(js, x, S.NFEAT, missing=-999.0, approximate=approximate, ntree_limit=limit)
        if approximate:
            same(got, restated, f"ntree_limit {limit}")
        else:
            ref64 = cs.treeshap64(d[:limit], base, x, -999.0, S.NFEAT)
            bound_exact(got, ref64, restated, max_len, f"ntree_limit {limit}")
        same(got[:, -1:], restated[:, -1:], f"bias, ntree_limit {limit}")


# ---- launch-shape boundaries: small boosters, big batches ----

def _check_big(b, js, x, nfeat, approximate, boundary_tiles, seed):
    """A big batch: the rows of every listed tile computed alone (small batches, split over waves) give the same bits
    as inside the big batch; a seeded sample of 300 rows per 8 192 tiles against the restatement."""
    whole = b.predict_contribs(capi.DMatrix(x, missing=-999.0), approximate=approximate)
    tiles = (len(x) + TILE - 1) // TILE
    for t in boundary_tiles:
        lo, hi = max(0, t * TILE), min(len(x), (t + 1) * TILE)
        alone = b.predict_contribs(capi.DMatrix(np.ascontiguousarray(x[lo:hi]), missing=-999.0),
                                   approximate=approximate)
        same(alone, whole[lo:hi], f"tile {t} of {tiles}")
    rng = np.random.default_rng(seed)
    for l0 in range(0, tiles, 8192):
        r0, r1 = l0 * TILE, min(len(x), (l0 + 8192) * TILE)
        pick = np.sort(rng.choice(np.arange(r0, r1), min(300, r1 - r0), replace=False))
        ref = synth.contribs_cpu(js, x[pick], nfeat, missing=-999.0, approximate=approximate)
        if approximate:
            same(whole[pick], ref, f"sample of launch {l0 // 8192}")
        else:
            assert cs.within(whole[pick], ref.astype(np.float64)) <= 1.0


def test_split_direct_switch():
    """262 144 rows (4 096 tiles) split over waves, 262 145 go direct; rows on either side of the tile boundary alone
    give the same bits as inside either batch."""
    rng = np.random.default_rng(51)
    js, _, _ = cs.random_booster(rng, 10, 8, 6, 0.2)
    x = cs.random_rows(rng, 4096 * TILE + 1, 8)
    b = capi.Booster(model_buffer=js)
    assert synth.contribs_plan(4096 * TILE, 8, 10) == (True, 2, 5, 0)
    assert synth.contribs_plan(4096 * TILE + 1, 8, 10) == (False, 0, 0, 1)
    for approximate in (False, True):
        _check_big(b, js, np.ascontiguousarray(x[:-1]), 8, approximate, [0, 4094, 4095], 1)
        _check_big(b, js, x, 8, approximate, [0, 4094, 4095, 4096], 2)


def test_part_budget():
    """128 features, 16 trees: 2 048 tiles need exactly 1 GiB of per-tree partials and split; one tile more goes
    direct."""
    rng = np.random.default_rng(52)
    js, _, _ = cs.random_booster(rng, 16, 128, 5, 0.2)
    x = cs.random_rows(rng, 2048 * TILE + 1, 128)
    b = capi.Booster(model_buffer=js)
    assert synth.contribs_plan(2048 * TILE, 128, 16) == (True, 4, 4, 0)
    assert synth.contribs_plan(2048 * TILE + 1, 128, 16) == (False, 0, 0, 1)
    for approximate in (False, True):
        _check_big(b, js, np.ascontiguousarray(x[:-1]), 128, approximate, [0, 2047], 3)
        _check_big(b, js, x, 128, approximate, [0, 2047, 2048], 4)


def test_exact_direct_launches_past_8192_tiles():
    """8 196 tiles, the last of 17 rows: exact mode's direct form in two launches, the second from tile 8 192 on."""
    rng = np.random.default_rng(53)
    js, _, _ = cs.random_booster(rng, 3, 8, 6, 0.2)
    n = 8195 * TILE + 17
    x = cs.random_rows(rng, n, 8)
    b = capi.Booster(model_buffer=js)
    assert synth.contribs_plan(n, 8, 3) == (False, 0, 0, 2)
    _check_big(b, js, x, 8, False, [0, 8190, 8191, 8192, 8193, 8194, 8195], 5)


# ---- feature counts ----

def test_feature_counts(torch_cuda):
    """F = 1 and F = 128 (a block's two [F][64] tiles fill its 64 KiB of LDS), both modes; F = 129 is refused; fewer
    columns than features in the device form and in approximate mode (the absent columns are missing)."""
    torch = torch_cuda
    rng = np.random.default_rng(61)
    for nfeat, ntree, depth in ((1, 4, 3), (128, 6, 9)):
        js, trees, base = cs.random_booster(rng, ntree, nfeat, depth, 0.2)
        b = capi.Booster(model_buffer=js)
        x = cs.random_rows(rng, 300, nfeat)
        for missing in (-999.0, float("nan")):
            got = every_form(torch, b, x, missing)
            assert cs.within(got, cs.treeshap64(trees, base, x, missing, nfeat)) <= 1.0, (nfeat, missing)
            ap = every_form(torch, b, x, missing, approximate=True)
            same(ap, synth.contribs_cpu(js, x, nfeat, missing=missing, approximate=True), f"F = {nfeat}")
        if nfeat == 128:
            part = np.ascontiguousarray(x[:, :100])
            for approximate in (False, True):
                got = every_form(torch, b, part, -999.0, approximate)
                if approximate:
                    same(got, synth.contribs_cpu(js, part, nfeat, missing=-999.0, approximate=True), "ncol < F")
                    assert cs.within(got, cs.saabas64(trees, base, part, -999.0, nfeat)) <= 1.0
                else:
                    assert cs.within(got, cs.treeshap64(trees, base, part, -999.0, nfeat)) <= 1.0
    js, _, _ = cs.random_booster(rng, 2, 129, 4, 0.2)
    b = capi.Booster(model_buffer=js)
    x = cs.random_rows(rng, 64, 129)
    for approximate in (False, True):
        with pytest.raises(capi.OhxError, match="at most 128 features"):
            b.predict_contribs(capi.DMatrix(x, missing=-999.0), approximate=approximate)


# ---- model formats and objectives ----

def _with_objective(js, name, base_score):
    doc = json.loads(js)
    doc["learner"]["objective"] = {"name": name}
    doc["learner"]["learner_model_param"]["base_score"] = "%.9g" % base_score
    return json.dumps(doc).encode()


def test_formats_give_the_same_bits(torch_cuda):
    js = booster(10)[0]
    x = rows(10, float("nan"))
    for approximate in (False, True):
        want = every_form(torch_cuda, capi.Booster(model_buffer=js), x, np.nan, approximate)
        for fmt in ("binary", "ubj"):
            img = synth.convert_model(js, fmt).tobytes()
            got = every_form(torch_cuda, capi.Booster(model_buffer=img), x, np.nan, approximate)
            same(got, want, f"{fmt}, approximate={approximate}")


def test_objectives_start_the_bias_from_the_margin_base(torch_cuda):
    """binary:logistic (base 0.25) and count:poisson (base 0.5) start the bias column from ProbToMargin(base_score);
    a pre-1.0 legacy image (reg:linear) holds the margin itself.  Each against the restatement bit for bit and local
    accuracy against the oracle's option-mask-1 margin; an objective with no known margin base is refused, as predict
    refuses it."""
    js, trees, base, d, max_len = booster(2)
    x = rows(2, -999.0)
    images = {"binary:logistic": _with_objective(js, "binary:logistic", 0.25),
              "count:poisson": _with_objective(js, "count:poisson", 0.5),
              "reg:linear (< 1.0)": helpers.legacy_image(json.loads(js), version=(0, 0), objective="reg:linear",
                                                         base_score=0.375)}
    for what, img in images.items():
        b = capi.Booster(model_buffer=img)
        for approximate in (False, True):
            got = every_form(torch_cuda, b, x, -999.0, approximate)
            restated = synth.contribs_cpu(img, x, S.NFEAT, missing=-999.0, approximate=approximate)
            same(got[:, -1:], restated[:, -1:], f"bias, {what}")
            if approximate:
                same(got, restated, what)
            local_accuracy(got, img, x, -999.0, max_len, f"{what}, approximate={approximate}")
    # the bias is sum of root means + ProbToMargin(base_score): -log(1 / 0.25 - 1), log(0.5), and 0.375 as it stands
    means = float(synth.contribs_cpu(_with_objective(js, "reg:squarederror", 0.0), x[:1], S.NFEAT)[0, -1])
    for what, m in (("binary:logistic", -np.log(3.0)), ("count:poisson", np.log(0.5)), ("reg:linear (< 1.0)", 0.375)):
        bias = float(synth.contribs_cpu(images[what], x[:1], S.NFEAT)[0, -1])
        assert abs(bias - (means + m)) <= 2e-7 * (1.0 + abs(means) + abs(m)), what
    b = capi.Booster(model_buffer=_with_objective(js, "reg:made-up-loss", 0.5))
    with pytest.raises(capi.OhxError) as predict_err:
        b.predict(capi.DMatrix(x, missing=-999.0))
    for approximate in (False, True):
        with pytest.raises(capi.OhxError) as err:
            b.predict_contribs(capi.DMatrix(x, missing=-999.0), approximate=approximate)
        assert str(err.value) == str(predict_err.value)


# ---- +-inf in the host form ----

def test_inf_anywhere_in_the_row_is_refused(torch_cuda):
    """The host form of the call (OHXBoosterPredictContribs) on a device matrix, `missing` finite: +inf in a column no
    tree splits on, -inf in a row of a booster whose trees are all root leaves - refused by both modes in both shapes,
    as Booster.predict refuses the same matrix, and the next call on clean data succeeds (the flag was cleared).  With
    missing = +inf the same rows are accepted and +inf is missing.  (A host matrix holding +-inf is refused when it is
    made, XGDMatrixCreateFromMat.)"""
    torch = torch_cuda
    rng = np.random.default_rng(71)
    from tests.test_random_forests import random_tree
    unsplit, _, _ = cs.booster_from_trees(rng, [random_tree(rng, 6, 6, 0.2) for _ in range(8)], 8)
    leaves, _, _ = cs.booster_from_trees(rng, [([-1], [-1], [0], [0.25 * i], [0]) for i in range(3)], 8)
    clean = cs.random_rows(rng, 200, 8)
    t_clean = torch.from_numpy(clean).cuda()
    d_clean = capi.DMatrix(device_ptr=t_clean.data_ptr(), nrow=200, ncol=8, missing=-999.0)
    for js, (r, c, v) in ((unsplit, (5, 7, np.inf)), (unsplit, (130, 6, -np.inf)), (leaves, (3, 2, -np.inf))):
        x = clean.copy()
        x[r, c] = v
        with pytest.raises(capi.OhxError, match="Input data contains"):
            capi.DMatrix(x, missing=-999.0)
        t = torch.from_numpy(x).cuda()
        d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=200, ncol=8, missing=-999.0)
        b = capi.Booster(model_buffer=js)
        with pytest.raises(capi.OhxError, match="Input data contains"):
            b.predict(d)
        for split in ("auto", "off"):
            b.set_param("ohx_contribs_split", split)
            for approximate in (False, True):
                with pytest.raises(capi.OhxError, match="Input data contains"):
                    b.predict_contribs(d, approximate=approximate)
                ok = b.predict_contribs(d_clean, approximate=approximate)
                assert ok.shape == (200, 9) and np.all(np.isfinite(ok))
                if v > 0:      # missing = +inf: accepted, and +inf is missing (as NaN is)
                    y = x.copy()
                    y[r, c] = np.nan
                    ty = torch.from_numpy(y).cuda()
                    got = b.predict_contribs(capi.DMatrix(device_ptr=t.data_ptr(), nrow=200, ncol=8, missing=np.inf),
                                             approximate=approximate)
                    want = b.predict_contribs(capi.DMatrix(device_ptr=ty.data_ptr(), nrow=200, ncol=8,
                                                           missing=np.inf), approximate=approximate)
                    same(got, want, "+inf missing")
