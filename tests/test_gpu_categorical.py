"""Boosters with categorical splits on the GPU, everything bit for bit (docs/14_categorical.md): margins, values and leaf
ids against the numpy restatement of the routing table (tests/categorical_support.py) - host and device forms, the tile
and the direct kernel, both missing markers, fewer columns than features, ntree_limit, batches from one row to 262 144,
with and without a grid, bricks of a grid the rows start inside - the edge values at categorical nodes, the suffix twin against the CPU oracle, independence
of the batch, the capture refusal, and scikit-learn's categorical histogram trees as an outside walker."""
import json

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import categorical_support as CS
from tests import helpers

pytestmark = pytest.mark.gpu

NROWS = [1, 63, 64, 65, 10000, 262144]
KERNELS = {"auto": "predict_cat_tile_kernel", "direct": "predict_cat_direct_kernel<false>"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def img(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def booster(image, cat_kernel="auto"):
    b = capi.Booster(model_buffer=img(image))
    b.set_param("ohx_cat_kernel", cat_kernel)
    return b


def predict_host(image, rows, missing, option_mask=1, ntree_limit=0, cat_kernel="auto", grid=None):
    b = booster(image, cat_kernel)
    d = capi.DMatrix(rows, missing=missing)
    if grid is not None:
        d.set_grid(grid[0], grid[1], 0)
    out = b.predict(d, option_mask=option_mask, ntree_limit=ntree_limit)
    d.free()
    b.free()
    return out


def predict_device(torch, image, rows, missing, option_mask=1, ntree_limit=0, cat_kernel="auto", grid=None, width=1):
    b = booster(image, cat_kernel)
    t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
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


@pytest.fixture(scope="module")
def case():
    js, trees, cat_max = CS.make_booster(2024, 12)
    return js, trees, cat_max


_expected = {}


def expected(case, nrow, missing):
    """Rows and what the restatement makes of them, computed once per (size, missing marker)."""
    key = (nrow, "nan" if np.isnan(missing) else missing)
    if key not in _expected:
        js, trees, cat_max = case
        X = CS.rows(100 + nrow % 97, nrow, cat_max, missing=missing)
        margins, leaves = CS.predict(trees, CS.base_of(js), X, missing)
        _expected[key] = (X, margins, leaves)
    return _expected[key]


def same_bits(a, b):
    return np.array_equal(helpers.bits(a), helpers.bits(b))


@pytest.mark.parametrize("cat_kernel", sorted(KERNELS))
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("missing", [float("nan"), -999.0])
@pytest.mark.parametrize("nrow", NROWS)
def test_margins_values_and_leaf_ids_are_the_restatements(torch_cuda, case, nrow, missing, form, cat_kernel):
    js, trees, cat_max = case
    X, margins, leaves = expected(case, nrow, missing)
    T = len(trees)
    grids = [None] if nrow < 64 else [None, (8, 4)]                      # with and without OHXDMatrixSetGrid
    for grid in grids:
        for option_mask, want in ((1, margins), (0, margins), (16, leaves.reshape(-1))):
            if form == "host":
                got = predict_host(js, X, missing, option_mask, 0, cat_kernel, grid)
            else:
                got = predict_device(torch_cuda, js, X, missing, option_mask, 0, cat_kernel, grid,
                                     width=T if option_mask == 16 else 1)
            print("nrow %d missing %s %s %s grid %s option_mask %d: %d of %d words differ" %
                  (nrow, missing, form, cat_kernel, grid, option_mask,
                   int(np.count_nonzero(helpers.bits(got) != helpers.bits(want))), want.size))
            assert same_bits(got, want), (nrow, missing, form, cat_kernel, grid, option_mask)


@pytest.mark.parametrize("cat_kernel", sorted(KERNELS))
def test_the_symbols_name_the_new_kernels(case, cat_kernel):
    js, trees, cat_max = case
    b = booster(js, cat_kernel)
    d = capi.DMatrix(CS.rows(1, 300, cat_max), missing=float("nan"))
    assert b.kernel_symbols_for(d) == KERNELS[cat_kernel]
    assert b.kernel_symbol(CS.NFEAT) == KERNELS[cat_kernel]
    info = b.info()
    assert info["num_trees"] == len(trees)
    # the launch knobs of the numeric walks are accepted and select nothing here
    want = b.predict(d, option_mask=1)
    for name, value in (("ohx_kernel", "wide"), ("ohx_kernel", "ring"), ("ohx_tree_split", "4"), ("ohx_cluster", "on"),
                        ("ohx_defer_missing", "on"), ("ohx_brick", "4,4,4")):
        b.set_param(name, value)
        assert b.kernel_symbols_for(d) == KERNELS[cat_kernel]
        assert same_bits(b.predict(d, option_mask=1), want), (name, value)
    d.free()
    b.free()


@pytest.mark.parametrize("cat_kernel", sorted(KERNELS))
@pytest.mark.parametrize("missing", [float("nan"), -999.0])
def test_fewer_columns_than_features_and_ntree_limit(torch_cuda, case, cat_kernel, missing):
    js, trees, cat_max = case
    X = CS.rows(5, 1000, cat_max, missing=missing)
    T = len(trees)
    for ncol in (CS.NFEAT, 12, 1):
        Xc = np.ascontiguousarray(X[:, :ncol])
        for limit in (0, 5, T, T + 7):
            margins, leaves = CS.predict(trees, CS.base_of(js), Xc, missing, limit)
            assert same_bits(predict_host(js, Xc, missing, 1, limit, cat_kernel), margins), (ncol, limit)
            assert same_bits(predict_device(torch_cuda, js, Xc, missing, 1, limit, cat_kernel), margins), (ncol, limit)
            got = predict_host(js, Xc, missing, 16, limit, cat_kernel)
            assert got.size == leaves.size and np.array_equal(got.reshape(leaves.shape), leaves), (ncol, limit)
            got = predict_device(torch_cuda, js, Xc, missing, 16, limit, cat_kernel, width=leaves.shape[1])
            assert np.array_equal(got.reshape(leaves.shape), leaves), (ncol, limit)


@pytest.mark.parametrize("grid", [(12, 9, 50), (64, 64, 0), (5, 3, 7), (360, 2160, 1000)])
@pytest.mark.parametrize("brick", ["auto", "8,8,1", "2,2,16", "0,0,0"])
def test_bricks_of_a_grid_the_rows_start_inside(torch_cuda, case, grid, brick):
    """The tile kernel takes bricks of the grid the caller names (OHXDMatrixSetGrid), whatever row of the grid the matrix
    starts at and wherever it ends: every row is predicted once, with the same bits."""
    js, trees, cat_max = case
    X, margins, _ = expected(case, 10000, float("nan"))
    b = booster(js)
    b.set_param("ohx_brick", brick)
    t = torch_cuda.from_numpy(X).cuda()
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=len(X), ncol=X.shape[1], missing=float("nan"))
    d.set_grid(*grid)
    out = torch_cuda.full((len(X),), float("nan"), dtype=torch_cuda.float32, device="cuda")
    b.predict_device(d, out.data_ptr(), option_mask=1)
    torch_cuda.cuda.synchronize()
    b.check()
    assert same_bits(out.cpu().numpy(), margins), (grid, brick)
    d.free()
    b.free()


@pytest.mark.parametrize("nfeat", [100, 200])
def test_wide_boosters_tile_in_a_big_lds_allocation_or_fall_back_to_the_direct_kernel(torch_cuda, nfeat):
    """100 features: a block's four tiles take 100 KiB of LDS (more than the 64 KiB a launch gets unasked); 200 do not
    fit a CU's 160 KiB and the direct kernel takes the margins."""
    js, trees, cat_max = CS.make_booster(77, 6, nfeat=nfeat)
    X = CS.rows(78, 3000, cat_max, nfeat=nfeat)
    margins, leaves = CS.predict(trees, CS.base_of(js), X)
    b = booster(js)
    assert b.kernel_symbol(nfeat) == ("predict_cat_tile_kernel" if nfeat == 100 else "predict_cat_direct_kernel<false>")
    b.free()
    assert same_bits(predict_host(js, X, float("nan")), margins)
    assert same_bits(predict_device(torch_cuda, js, X, float("nan")), margins)
    assert np.array_equal(predict_host(js, X, float("nan"), 16).reshape(leaves.shape), leaves)


@pytest.mark.parametrize("cat_kernel", sorted(KERNELS))
@pytest.mark.parametrize("missing", [float("nan"), -999.0, float("inf")])
def test_edge_values_at_categorical_nodes(torch_cuda, case, cat_kernel, missing):
    """-1, -0.5, -0.0, 0, M, M + 0.999, Size - 1, Size, Size + 1, 2.7, 3e9, 1e30, NaN and `missing` in every categorical
    column; with missing = inf, +-inf too (allowed: +inf is the missing marker, -inf a value below zero)."""
    js, trees, cat_max = case
    extra = (float("inf"), float("-inf")) if np.isinf(missing) else ()
    X = CS.edge_rows(9, cat_max, missing=missing, extra=extra)
    margins, leaves = CS.predict(trees, CS.base_of(js), X, missing)
    assert same_bits(predict_host(js, X, missing, 1, 0, cat_kernel), margins)
    assert same_bits(predict_device(torch_cuda, js, X, missing, 1, 0, cat_kernel), margins)
    assert np.array_equal(predict_host(js, X, missing, 16, 0, cat_kernel).reshape(leaves.shape), leaves)
    # one tree whose root is categorical on each feature in turn: the leaf says which way the edge value went
    for f, m in cat_max.items():
        for dl in (0, 1):
            t = CS.Tree()
            root = t.node()
            l, r = t.split(root)
            t.feat[root], t.stype[root], t.dl[root], t.cats[root], t.cond[root] = f, 1, dl, [m], float("nan")
            t.cond[l], t.cond[r] = -1.0, 1.0
            one = CS.booster_json([t], 0.0, CS.NFEAT, cat_max)
            vals = CS.edge_values(m, missing) + list(extra)
            R = np.zeros((len(vals), CS.NFEAT), dtype=np.float32)
            R[:, f] = np.array(vals, dtype=np.float32)
            want, _ = CS.predict([t], 0.0, R, missing)
            # by hand, from the table: only M itself (and M + 0.999, which truncates to M) is in the set {M}
            size = CS.capacity(m)
            by_hand = []
            for v in np.array(vals, dtype=np.float32):
                is_missing = np.isnan(v) or (not np.isnan(missing) and v == np.float32(missing))
                if is_missing or v < 0 or v >= size:
                    by_hand.append(-1.0 if dl else 1.0)
                else:
                    by_hand.append(1.0 if int(v) == m else -1.0)
            assert np.array_equal(want, np.array(by_hand, dtype=np.float32)), (f, m, dl)
            assert same_bits(predict_host(one, R, missing, 1, 0, cat_kernel), want), (f, m, dl)


@pytest.mark.parametrize("cat_kernel", sorted(KERNELS))
def test_infinities_with_a_finite_missing_marker(torch_cuda, case, cat_kernel):
    """The host form refuses the matrix, as for every booster; the device form raises the flag OHXBoosterCheck sees -
    wherever in the row the infinity sits, walked or not."""
    torch = torch_cuda
    js, trees, cat_max = case
    for missing in (float("nan"), -999.0):
        for col in (0, 1, CS.NFEAT - 1):
            for v in (float("inf"), float("-inf")):
                X = CS.rows(3, 200, cat_max, missing=missing)
                X[137, col] = v
                with pytest.raises(capi.OhxError, match="inf"):
                    capi.DMatrix(X, missing=missing)
                b = booster(js, cat_kernel)
                t = torch.from_numpy(X).cuda()
                d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=len(X), ncol=X.shape[1], missing=missing)
                out = torch.zeros(len(X), dtype=torch.float32, device="cuda")
                b.predict_device(d, out.data_ptr(), option_mask=1)
                torch.cuda.synchronize()
                with pytest.raises(capi.OhxError, match="inf"):
                    b.check()
                b.check()                                                   # the flag was taken down
                d.free()
                b.free()


def test_the_suffix_twin_against_the_oracle(torch_cuda):
    """A booster whose sets are suffixes {k, ..., M} routes rows inside [0, M + 1) as its numeric twin does - a model the
    CPU oracle reads.  The oracle's margins on the twin are the new kernels' on the categorical booster, and the
    product's own default kernel on the twin gives them too."""
    js, trees, cat_max = CS.make_booster(4711, 16, suffix=True)
    tw = CS.twin(js, trees, cat_max)
    assert capi.Booster(model_buffer=img(tw)).num_categorical_splits() == 0
    for missing in (float("nan"), -999.0):
        X = CS.rows(4712, 20000, cat_max, missing=missing, wild=False)
        CS.assert_in_twin_range(X, cat_max, missing)
        want = helpers.oracle_predict(synth.convert_model(tw, "binary"), X, missing, option_mask=1)
        for cat_kernel in sorted(KERNELS):
            assert same_bits(predict_host(js, X, missing, 1, 0, cat_kernel), want), cat_kernel
            assert same_bits(predict_device(torch_cuda, js, X, missing, 1, 0, cat_kernel), want), cat_kernel
        b = capi.Booster(model_buffer=img(tw))
        d = capi.DMatrix(X, missing=missing)
        assert not b.kernel_symbols_for(d).startswith("predict_cat")
        assert same_bits(b.predict(d, option_mask=1), want)
        d.free()
        b.free()


def test_a_row_does_not_depend_on_its_batch(torch_cuda, case):
    js, trees, cat_max = case
    X, margins, _ = expected(case, 262144, float("nan"))
    whole = predict_device(torch_cuda, js, X, float("nan"))
    assert same_bits(whole, margins)
    rng = np.random.default_rng(5)
    picks = np.concatenate([[0, 63, 64, 262143], rng.integers(0, len(X), 60)])
    b = booster(js)
    bd = booster(js, "direct")
    for r in picks:
        for bb in (b, bd):
            d = capi.DMatrix(np.ascontiguousarray(X[r:r + 1]), missing=float("nan"))
            alone = bb.predict(d, option_mask=1)
            d.free()
            assert same_bits(alone, whole[r:r + 1]), int(r)
    # ... nor on where in a batch it stands: a shuffled batch
    perm = rng.permutation(5000)
    d = capi.DMatrix(np.ascontiguousarray(X[perm]), missing=float("nan"))
    assert same_bits(b.predict(d, option_mask=1), whole[perm])
    d.free()
    b.free()
    bd.free()


def test_capture_of_a_categorical_device_predict_is_refused(torch_cuda, case):
    torch = torch_cuda
    js, trees, cat_max = case
    X = CS.rows(8, 256, cat_max)
    rows = torch.from_numpy(X).cuda()
    out = torch.zeros(256, dtype=torch.float32, device="cuda")
    b = booster(js)
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=256, ncol=CS.NFEAT, missing=float("nan"))
    b.predict_device(d, out.data_ptr(), option_mask=1)
    torch.cuda.synchronize()
    before = out.clone()
    out.zero_()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="categorical"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.predict_device(d, out.data_ptr(), option_mask=1, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not out.any()                                                   # nothing was enqueued
    b.check()
    b.predict_device(d, out.data_ptr(), option_mask=1)
    torch.cuda.synchronize()
    assert torch.equal(out, before)


def test_other_objectives_keep_their_refusal_for_values(case):
    js, trees, cat_max = CS.make_booster(2024, 3, objective="binary:logistic")
    doc = json.loads(js)
    doc["learner"]["learner_model_param"]["base_score"] = "0.5"
    image = json.dumps(doc).encode()
    X = CS.rows(1, 100, cat_max)
    with pytest.raises(capi.OhxError, match="prediction transform"):
        predict_host(image, X, float("nan"), option_mask=0)
    margins, _ = CS.predict(trees, 0.0, X)                                 # ProbToMargin(0.5) = 0
    assert same_bits(predict_host(image, X, float("nan"), option_mask=1), margins)


# ---------------------------------------------------------------- scikit-learn's categorical histogram trees

def transcribe_hist_tree(nodes, raw_left_cat_bitsets, known_categories):
    """One scikit-learn TreePredictor as a single-tree booster (base 0).  Numeric nodes keep their orientation: x <= thr
    becomes x < the next float32 above thr, default_left = missing_go_to_left.  At a CATEGORICAL node the children are
    swapped - scikit-learn sends a category of its set left, xgboost right - default_left = not missing_go_to_left, and
    the set S is the set bits of the node's raw_left_cat_bitsets row.

    One case that rule cannot transcribe: xgboost sends a category at or beyond Size = 32 * ceil((max(S) + 1) / 32) to
    the DEFAULT child, scikit-learn has no such capacity and sends every category outside its set right.  Where a node
    has missing_go_to_left = 1 and the feature has a known category >= Size (a left set {0..52} of a feature with
    categories up to 69), the swapped node would send categories 64..69 the way NaN goes - scikit-learn's left.  Such a
    node is written the other way round, which is exact for it: no swap, S = the feature's known categories outside
    the left set, default_left = missing_go_to_left (now every category beyond S's capacity is one of the left set and
    goes left with NaN).  The same for a node whose left set is empty (only NaN goes left): an empty set has no file
    form.  Every other categorical node follows the rule above; `complemented` counts the exceptions.
    known_categories: feature -> the categories scikit-learn's bin mapper knows."""
    t = CS.Tree()
    t.complemented = 0
    new_of = {0: t.node()}
    order = [0]
    for old in order:
        nd = nodes[old]
        new = new_of[old]
        if nd["is_leaf"]:
            t.cond[new] = float(np.float32(nd["value"]))
            continue
        l, r = t.split(new)
        f = int(nd["feature_idx"])
        t.feat[new] = f
        if nd["is_categorical"]:
            words = raw_left_cat_bitsets[int(nd["bitset_idx"])]
            left_set = [c for c in range(32 * len(words)) if (int(words[c >> 5]) >> (c & 31)) & 1]
            # (an empty left set - only NaN goes left - has no capacity at all, and no file form: a segment of size 0)
            beyond = [c for c in known_categories[f] if not left_set or c >= CS.capacity(max(left_set))]
            t.stype[new], t.cond[new] = 1, float("nan")
            if nd["missing_go_to_left"] and beyond:
                t.complemented += 1
                new_of[int(nd["left"])], new_of[int(nd["right"])] = l, r
                t.dl[new] = 1
                t.cats[new] = [c for c in known_categories[f] if c not in left_set]
                order += [int(nd["left"]), int(nd["right"])]
            else:
                new_of[int(nd["right"])], new_of[int(nd["left"])] = l, r    # swapped
                t.dl[new] = 0 if nd["missing_go_to_left"] else 1
                t.cats[new] = left_set
                order += [int(nd["right"]), int(nd["left"])]
        else:
            new_of[int(nd["left"])], new_of[int(nd["right"])] = l, r
            t.dl[new] = int(nd["missing_go_to_left"])
            thr = float(nd["num_threshold"])
            down = np.float32(thr)
            if float(down) > thr:
                down = np.nextafter(down, np.float32(-np.inf))
            t.cond[new] = float(np.nextafter(down, np.float32(np.inf)))     # smallest float32 strictly above thr
            order += [int(nd["left"]), int(nd["right"])]
    return t


def known_categories_of(mapper):
    bitsets, f_idx_map = mapper.make_known_categories_bitsets()
    out = {}
    for f, row in enumerate(f_idx_map):
        if mapper.is_categorical_[f]:
            words = bitsets[int(row)]
            out[f] = [c for c in range(32 * len(words)) if (int(words[c >> 5]) >> (c & 31)) & 1]
    return out


def hist_case():
    """(predictors, bin mapper, rows): 5 trees on 6 features, the first two categorical (0..69 and 0..11), 5 % NaN.
    The categorical columns come first because scikit-learn moves them there before it bins (its trees number the
    features of THAT order): with them in front the order is the caller's."""
    from sklearn.ensemble import HistGradientBoostingRegressor
    rng = np.random.default_rng(0)
    n = 4000
    X = rng.normal(size=(n, 6)).astype(np.float32)
    X[:, 0] = rng.integers(0, 70, n)
    X[:, 1] = rng.integers(0, 12, n)
    y = np.sin(X[:, 0]) + (X[:, 1] % 3) + X[:, 2]
    X[rng.random(X.shape) < 0.05] = np.nan
    m = HistGradientBoostingRegressor(max_iter=5, max_depth=6, categorical_features=[0, 1], random_state=0).fit(X, y)
    predictors = [p[0] for p in m._predictors]
    for p in predictors:
        _ = p.nodes, p.raw_left_cat_bitsets
    return predictors, m._bin_mapper, X[:1500]


def test_scikit_learn_categorical_histogram_trees(torch_cuda):
    """May skip (private attributes of scikit-learn); no other test of this file may."""
    pytest.importorskip("sklearn")
    try:
        predictors, mapper, X = hist_case()
        known = mapper.make_known_categories_bitsets()
        categories = known_categories_of(mapper)
    except (AttributeError, ImportError) as e:
        pytest.skip("this scikit-learn does not expose its histogram trees (_predictors, nodes, raw_left_cat_bitsets, "
                    "make_known_categories_bitsets, is_categorical_): %s" % e)
    assert np.isnan(X).any()
    assert categories == {0: list(range(70)), 1: list(range(12))}
    ncat = complemented = 0
    for p in predictors:
        t = transcribe_hist_tree(p.nodes, p.raw_left_cat_bitsets, categories)
        ncat += len(t.cats)
        complemented += t.complemented
        one = CS.booster_json([t], 0.0, X.shape[1], {0: 69, 1: 11})
        want = p.predict(X.astype(np.float64), *known, 1).astype(np.float32)
        restated, _ = CS.predict([t], 0.0, X)
        bad = int(np.count_nonzero(helpers.bits(restated) != helpers.bits(want)))
        print("scikit-learn tree: %d categorical nodes, %d of %d rows differ in the restatement" % (len(t.cats), bad, len(X)))
        for cat_kernel in sorted(KERNELS):
            got = predict_host(one, X, float("nan"), 1, 0, cat_kernel)
            assert same_bits(got, want), cat_kernel
    print("%d categorical nodes, %d of them written as complements" % (ncat, complemented))
    assert ncat > 0 and complemented < ncat
