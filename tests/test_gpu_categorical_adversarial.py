"""The categorical kernels on adversarial boosters and past their launch caps, everything bit for bit against the
restatement (docs/14_categorical.md 14.6): tests/categorical_support.py make_adversarial - root leaves beside depth-30
chains, several capacities on one path, repeated, full and word-edge sets, the category 2**24 - 1 - with random rows
and category_tie_rows; batches of more than twice the rows one trip of a kernel's grid-stride loop takes (the caps are
computed here from the device's CU count), where a wave refills its LDS tile; 160 features (a block's 160 KiB of dynamic
LDS, the last count the tile kernel takes) and 161; bricks of a grid on such a batch.  Host and device forms,
`ohx_cat_kernel` auto and direct, NaN and -999.0 as the missing marker."""
import numpy as np
import pytest

from quickchem_amd import capi
from tests import categorical_support as CS
from tests import helpers
from tests.test_gpu_categorical import KERNELS, booster, predict_device, predict_host, same_bits

pytestmark = pytest.mark.gpu

MISSING = [float("nan"), -999.0]
CU_LDS_BYTES = 163840                                   # categorical.hip kCuLdsBytes


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def num_cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def tile_cap(torch, nfeat):
    """An upper bound on the rows one trip of predict_cat_tile_kernel takes (launch_predict_cat): at most
    num_cus * blocks_per_cu blocks of four 64-row tiles, and blocks_per_cu cannot exceed what the LDS (4 * nfeat * 256
    bytes a block) or the 8 blocks of 4 waves a CU holds allow."""
    lds_bytes = 4 * nfeat * 256
    return num_cus(torch) * min(8, CU_LDS_BYTES // lds_bytes) * 256


def direct_cap(torch):
    """Rows one trip of predict_cat_direct_kernel takes: num_cus * 8 blocks of 256 lanes."""
    return num_cus(torch) * 8 * 256


def key(missing):
    return "nan" if np.isnan(missing) else missing


def predict(torch, form, image, rows, missing, option_mask=1, ntree_limit=0, cat_kernel="auto", grid=None, width=1):
    if form == "host":
        return predict_host(image, rows, missing, option_mask, ntree_limit, cat_kernel, grid)
    return predict_device(torch, image, rows, missing, option_mask, ntree_limit, cat_kernel, grid, width)


# ---------------------------------------------------------------- the adversarial boosters

_small = {}


def small_case(ntree):
    """The booster of `ntree` trees, its rows (random ones, with both missing markers in them, and tie rows) and the
    restatement of every (missing, ntree_limit) asked for."""
    if ntree not in _small:
        js, trees, cat_max = CS.make_adversarial(700 + ntree, ntree)
        X = np.concatenate([CS.rows(ntree, 800, cat_max, missing=-999.0),
                            CS.category_tie_rows(np.random.default_rng(ntree), trees, 350, cat_max)])
        _small[ntree] = (js, trees, X, {})
    return _small[ntree]


def small_expected(ntree, missing, limit):
    js, trees, X, memo = small_case(ntree)
    if (key(missing), limit) not in memo:
        memo[(key(missing), limit)] = CS.predict(trees, CS.base_of(js), X, missing, limit, walker=CS.walk_sparse)
    return memo[(key(missing), limit)]


def limits_for(ntree):
    """ntree_limit values that make the walked count 1, even and odd (0 = all trees)."""
    return sorted(k for k in {0, 1, 2, 3, ntree - 1, ntree + 4} if k >= 0)


@pytest.mark.parametrize("cat_kernel", sorted(KERNELS))
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("ntree", [1, 2, 3, 5, 10, 33])
def test_margins_and_leaf_ids_of_the_adversarial_boosters(torch_cuda, ntree, missing, form, cat_kernel):
    js, trees, X, _ = small_case(ntree)
    walked = set()
    for limit in limits_for(ntree):
        margins, leaves = small_expected(ntree, missing, limit)
        walked.add(leaves.shape[1])
        got = predict(torch_cuda, form, js, X, missing, 1, limit, cat_kernel)
        print("ntree %d limit %d missing %s %s %s: %d of %d margins differ" %
              (ntree, limit, missing, form, cat_kernel, int(np.count_nonzero(helpers.bits(got) != helpers.bits(margins))),
               len(X)))
        assert same_bits(got, margins), (ntree, limit)
        got = predict(torch_cuda, form, js, X, missing, 16, limit, cat_kernel, width=leaves.shape[1])
        assert got.size == leaves.size and np.array_equal(got.reshape(leaves.shape), leaves), (ntree, limit)
    assert 1 in walked and ntree in walked
    if ntree >= 3:
        assert {w & 1 for w in walked} == {0, 1}


# ---------------------------------------------------------------- the largest category

MAXCAT_VALUES = [16777215.0, 16777214.0, 16777216.0, 8388607.5, 3e9, float("nan"), 0.0, 3.0, 40.0, 41.0, -0.0]


@pytest.mark.parametrize("cat_kernel", sorted(KERNELS))
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("missing", MISSING)
def test_the_largest_category_on_the_device(torch_cuda, missing, form, cat_kernel):
    """Category 2**24 - 1: a node of 524 288 set words and Size = 2**24, the last integer a float32 holds exactly.  Its
    set is {0, 3, 40, 2**24 - 1}; the left child splits the same column numerically at 8388608.  Node ids: 0 the root,
    1 and 2 its children, 3 and 4 the children of 1."""
    for ntree in (1, 4):
        js, trees, cat_max = CS.make_adversarial(90 + ntree, ntree, maxcat=True)
        t = trees[-1]
        assert t.kind == "maxcat" and max(t.cats[0]) == 2 ** 24 - 1 and t.feat[0] == t.feat[1] == 1
        assert sorted(t.cats[0]) == [0, 3, 40, 2 ** 24 - 1] and t.cond[1] == 8388608.0
        root_default = 1 if t.dl[0] else 2
        below = {1: 4, 2: 2}                                       # where a value >= 8388608 ends up from that child
        by_hand = {16777215.0: 2,                                  # a member
                   16777214.0: 4,                                  # inside Size, no member: left, then not < 8388608
                   16777216.0: below[root_default],                # == Size: outside, the default child
                   8388607.5: 3,                                   # (int) 8388607: no member: left, then < 8388608
                   3e9: below[root_default],
                   "nan": {1: 3 if t.dl[1] else 4, 2: 2}[root_default],
                   0.0: 2, 3.0: 2, 40.0: 2, 41.0: 3, -0.0: 2}
        X = CS.rows(5, len(MAXCAT_VALUES), cat_max, p_missing=0.0, wild=False)
        X[:, 1] = np.array(MAXCAT_VALUES, dtype=np.float32)
        margins, leaves = CS.predict(trees, CS.base_of(js), X, missing, walker=CS.walk_sparse)
        want = [by_hand["nan" if np.isnan(v) else v] for v in MAXCAT_VALUES]
        assert list(leaves[:, -1]) == want
        got = predict(torch_cuda, form, js, X, missing, 16, 0, cat_kernel, width=ntree).reshape(leaves.shape)
        print("ntree %d: leaves of the 2**24 - 1 tree %s, by hand %s" % (ntree, list(got[:, -1]), want))
        assert list(got[:, -1]) == want
        assert np.array_equal(got, leaves)
        assert same_bits(predict(torch_cuda, form, js, X, missing, 1, 0, cat_kernel), margins)
        if ntree == 1:
            leaf_value = np.array(t.cond, dtype=np.float32)[np.array(want)]
            assert same_bits(margins, (CS.base_of(js) + leaf_value).astype(np.float32))
        # ... and among random rows of that column, which spread over all of [0, 2**24)
        R = np.concatenate([CS.rows(6, 3000, cat_max, missing=missing),
                            CS.category_tie_rows(np.random.default_rng(2), trees[-1:], 300, cat_max)])
        margins, leaves = CS.predict(trees, CS.base_of(js), R, missing, walker=CS.walk_sparse)
        assert len(np.unique(leaves[:, -1])) == 3
        assert same_bits(predict(torch_cuda, form, js, R, missing, 1, 0, cat_kernel), margins)
        got = predict(torch_cuda, form, js, R, missing, 16, 0, cat_kernel, width=ntree)
        assert np.array_equal(got.reshape(leaves.shape), leaves)


# ---------------------------------------------------------------- past the launch caps

_big = {}
# six trees for the wide boosters: the lopsided ones split numeric features all over the width, the others only the
# categorical features, which are the first odd ones
WIDE_KINDS = ["leaf", "chain30", "lopsided", "lopsided", "full_cat", "mixed_capacity"]


def big_case(nfeat, ntree, nrow):
    """An adversarial booster of `nfeat` features and at least `nrow` rows for it: random rows holding NaN and -999.0
    (a missing value or a value below zero, by the marker of the call), tie rows at both ends of the batch - the first
    and the last trip of the kernels' loops.  The restatement is made once per missing marker, for the largest row
    count asked for; a shorter batch is a prefix of it."""
    have = _big.get((nfeat, ntree))
    if have is None or len(have[2]) < nrow:
        js, trees, cat_max = CS.make_adversarial(40 + nfeat, ntree, nfeat=nfeat, kinds=None if nfeat == CS.NFEAT else WIDE_KINDS)
        if nfeat != CS.NFEAT:
            assert max(max(t.feat) for t in trees) >= nfeat - 20         # the last columns of a wide tile are read
        ties = CS.category_tie_rows(np.random.default_rng(nfeat), trees, 600, cat_max, nfeat=nfeat)
        X = CS.rows(nfeat, nrow, cat_max, nfeat=nfeat, missing=-999.0)
        X[:300], X[-300:] = ties[:300], ties[300:]
        _big[(nfeat, ntree)] = (js, trees, X, {})
    return _big[(nfeat, ntree)]


def big_expected(nfeat, ntree, missing, ncol=None):
    js, trees, X, memo = _big[(nfeat, ntree)]
    k = (key(missing), ncol)
    if k not in memo:
        memo[k] = CS.predict(trees, CS.base_of(js), X if ncol is None else X[:, :ncol], missing, walker=CS.walk_sparse)
    return memo[k]


def rows_past(cap):
    """More than twice the cap, and no multiple of 64: the last tile is short."""
    n = 2 * cap + 3 * 64 + 37
    assert n > 2 * cap and n % 64 != 0
    return n


def trip_rows(cap, nrow):
    """A handful of rows of each of the (at least three) trips."""
    return [0, 70, cap - 1, cap, cap + 3, cap + cap // 2, 2 * cap - 1, 2 * cap, 2 * cap + 65, nrow - 1]


def check_rows_alone(image, X, whole, picks, missing, cat_kernel):
    b = booster(image, cat_kernel)
    for r in picks:
        d = capi.DMatrix(np.ascontiguousarray(X[r:r + 1]), missing=missing)
        alone = b.predict(d, option_mask=1)
        d.free()
        assert same_bits(alone, whole[r:r + 1]), int(r)
    b.free()


def check_inf_in_the_last_trip(torch, image, X, nrow, missing, cat_kernel, grid=None):
    """Device form: +-inf in a row of the last trip raises the flag OHXBoosterCheck reports."""
    for v, col in ((float("inf"), X.shape[1] - 1), (float("-inf"), 0)):
        t = torch.from_numpy(np.ascontiguousarray(X[:nrow])).cuda()
        t[nrow - 5, col] = v
        b = booster(image, cat_kernel)
        d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=nrow, ncol=X.shape[1], missing=missing)
        if grid is not None:
            d.set_grid(grid[0], grid[1], 0)
        out = torch.zeros(nrow, dtype=torch.float32, device="cuda")
        b.predict_device(d, out.data_ptr(), option_mask=1)
        torch.cuda.synchronize()
        with pytest.raises(capi.OhxError, match="inf"):
            b.check()
        b.check()
        d.free()
        b.free()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("missing", MISSING)
@pytest.mark.parametrize("case", ["tile27", "tile27_grid", "tile100", "direct", "direct_leaf"])
def test_past_the_launch_caps(torch_cuda, case, missing, form):
    """Every thread takes a second and a third trip of its kernel's grid-stride loop; in the tile kernel a wave refills
    the LDS tile it has just walked, and the lanes of the last, short tile refill theirs with zeros."""
    nfeat, ntree = (100, 6) if case == "tile100" else (CS.NFEAT, 10)
    cat_kernel = "direct" if case.startswith("direct") else "auto"
    cap = direct_cap(torch_cuda) if cat_kernel == "direct" else tile_cap(torch_cuda, nfeat)
    nrow = rows_past(cap)
    assert nrow > 2 * cap
    # the 27-feature cases share one booster and one batch, made for the largest of them
    big_case(nfeat, ntree, nrow if nfeat != CS.NFEAT else rows_past(max(direct_cap(torch_cuda), tile_cap(torch_cuda, nfeat))))
    js, trees, X, _ = _big[(nfeat, ntree)]
    margins, leaves = big_expected(nfeat, ntree, missing)
    X = X[:nrow]
    grid = (8, 4) if case == "tile27_grid" else None
    b = booster(js, cat_kernel)
    assert b.kernel_symbol(nfeat) == KERNELS[cat_kernel]
    b.free()
    if case == "direct_leaf":
        L = 5
        got = predict(torch_cuda, form, js, X, missing, 16, L, cat_kernel, width=L).reshape(nrow, L)
        bad = int(np.count_nonzero(got != leaves[:nrow, :L]))
        print("%s %s missing %s: %d rows (cap %d), %d of %d leaf ids differ" % (case, form, missing, nrow, cap, bad, got.size))
        assert bad == 0
        return
    got = predict(torch_cuda, form, js, X, missing, 1, 0, cat_kernel, grid)
    bad = np.nonzero(helpers.bits(got) != helpers.bits(margins[:nrow]))[0]
    print("%s %s missing %s: %d rows (cap %d), %d margins differ, the first at rows %s" %
          (case, form, missing, nrow, cap, len(bad), bad[:5]))
    assert len(bad) == 0
    if form == "device":
        check_inf_in_the_last_trip(torch_cuda, js, X, nrow, missing, cat_kernel, grid)
    else:
        check_rows_alone(js, X, got, trip_rows(cap, nrow), missing, cat_kernel)


# ---------------------------------------------------------------- 160 and 161 features

@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("missing", MISSING)
def test_160_features_tile_in_all_of_a_cus_lds(torch_cuda, missing, form):
    """160 features: 4 waves * 160 * 256 bytes = 163 840 bytes of DYNAMIC LDS, all a CU has, one block a CU."""
    nfeat, ntree = 160, 6
    cap = tile_cap(torch_cuda, nfeat)
    assert cap == num_cus(torch_cuda) * 256
    nrow = rows_past(cap)
    assert nrow > 2 * cap
    js, trees, X, _ = big_case(nfeat, ntree, nrow)
    margins, _ = big_expected(nfeat, ntree, missing)
    b = booster(js)
    assert b.kernel_symbol(nfeat) == "predict_cat_tile_kernel"
    b.free()
    got = predict(torch_cuda, form, js, X[:nrow], missing)
    bad = np.nonzero(helpers.bits(got) != helpers.bits(margins[:nrow]))[0]
    print("160 features %s missing %s: %d rows (cap %d), %d margins differ %s" % (form, missing, nrow, cap, len(bad), bad[:5]))
    assert len(bad) == 0
    # fewer columns than features: the fill writes NaN into the rest of the tile on every trip
    ncol = 100
    few, _ = big_expected(nfeat, ntree, missing, ncol)
    Xc = np.ascontiguousarray(X[:nrow, :ncol])
    assert same_bits(predict(torch_cuda, form, js, Xc, missing), few[:nrow])
    assert not same_bits(few[:nrow], margins[:nrow])
    if form == "host":
        check_rows_alone(js, X, got, trip_rows(cap, nrow), missing, "auto")
    else:
        check_inf_in_the_last_trip(torch_cuda, js, X, nrow, missing, "auto")


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("missing", MISSING)
def test_161_features_go_to_the_direct_kernel(torch_cuda, missing, form):
    nfeat, ntree, nrow = 161, 6, 5000
    js, trees, X, _ = big_case(nfeat, ntree, nrow)
    margins, leaves = big_expected(nfeat, ntree, missing)
    b = booster(js)
    assert b.kernel_symbol(nfeat) == "predict_cat_direct_kernel<false>"
    b.free()
    assert same_bits(predict(torch_cuda, form, js, X, missing), margins)
    got = predict(torch_cuda, form, js, X, missing, 16, 0, "auto", width=ntree)
    assert np.array_equal(got.reshape(leaves.shape), leaves)
    few, _ = big_expected(nfeat, ntree, missing, 100)
    assert same_bits(predict(torch_cuda, form, js, np.ascontiguousarray(X[:, :100]), missing), few)


# ---------------------------------------------------------------- bricks on a batch beyond the cap

@pytest.mark.parametrize("grid", [(12, 9, 50), (64, 64, 0), (5, 3, 7), (360, 2160, 1000)])
@pytest.mark.parametrize("brick", ["auto", "8,8,1", "2,2,16", "0,0,0"])
def test_bricks_of_a_grid_on_a_batch_beyond_the_cap(torch_cuda, grid, brick):
    """The grids of test_gpu_categorical.py's brick test with the adversarial booster and more rows than one trip takes:
    a wave walks one brick, refills its tile and walks another."""
    torch = torch_cuda
    cap = tile_cap(torch, CS.NFEAT)
    nrow = cap + 5 * 64 + 11
    assert nrow > cap
    js, trees, X, _ = big_case(CS.NFEAT, 10, nrow)
    margins, _ = big_expected(CS.NFEAT, 10, float("nan"))
    b = booster(js)
    b.set_param("ohx_brick", brick)
    t = torch.from_numpy(np.ascontiguousarray(X[:nrow])).cuda()
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=nrow, ncol=X.shape[1], missing=float("nan"))
    d.set_grid(*grid)
    out = torch.full((nrow,), float("nan"), dtype=torch.float32, device="cuda")
    b.predict_device(d, out.data_ptr(), option_mask=1)
    torch.cuda.synchronize()
    b.check()
    assert same_bits(out.cpu().numpy(), margins[:nrow]), (grid, brick)
    d.free()
    b.free()
