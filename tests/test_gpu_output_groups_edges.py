"""The kernels of groups.hip at their edges (docs/13_output_groups.md 13.5): more elements than one trip of their
grid-stride loops takes, group shapes the first tests never made (G = 2, G = 64 with 10 trees, a group that is one root
leaf, groups emptied by ntree_limit), and the transforms on margins that are exact by construction - ties, one float32
step, the differences at which expf leaves the normal floats, then the denormals, -0.0 beside +0.0 - in the host and
the device form.  The reference for margins, leaf ids and contributions stays the decomposition into single-group
boosters, which the oracle pins."""
import numpy as np
import pytest

from quickchem_amd import capi
from tests import booster_shapes as S
from tests import helpers
from tests import output_groups_support as OG
from tests.test_gpu_output_groups import booster, expected_margins, predict_device, predict_host

pytestmark = pytest.mark.gpu

# groups.hip: kMaxBlocks * kBlock = 2048 * 256 elements is all one trip of a grid-stride loop takes, whatever the device
ONE_TRIP = 2048 * 256
NAN = float("nan")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def bits_equal(a, b):
    return np.array_equal(helpers.bits(np.asarray(a)), helpers.bits(np.asarray(b)))


def many_rows(seed, trees, n):
    """n rows drawn (with repeats) from 20 000 of booster_shapes.rows_for: tie rows are made one at a time."""
    base = S.rows_for(seed, trees, 20000, NAN)
    return np.ascontiguousarray(base[np.random.default_rng(seed).integers(0, len(base), n)])


# ---------------------------------------------------------------- past one trip of the loops

@pytest.fixture(scope="module")
def big():
    """G = 3, six trees, more than 2 * ONE_TRIP rows: rows, margins from the parts, and the host form's own."""
    nrow = 2 * ONE_TRIP + 77
    assert nrow >= 2 * ONE_TRIP and nrow % 256 != 0
    image, trees, info = OG.make_multi(911, 6, 3, "round_robin")
    rows = many_rows(3, trees, nrow)
    want = expected_margins(image, info, 3, rows, NAN)
    return image, trees, info, rows, want


@pytest.mark.parametrize("form", ["host", "device"])
def test_margins_softprob_and_softmax_past_one_trip(torch_cuda, big, form):
    image, trees, info, rows, want = big
    nrow = len(rows)
    assert nrow >= 2 * ONE_TRIP

    def run(img_, option_mask, width):
        if form == "host":
            return predict_host(img_, rows, NAN, option_mask).reshape(nrow, width)
        return predict_device(torch_cuda, img_, rows, NAN, option_mask, width=width).reshape(nrow, width)

    margins = run(image, 1, 3)
    bad = np.nonzero((helpers.bits(margins) != helpers.bits(want)).any(axis=1))[0]
    print("%s: %d rows, %d differ from the parts, the first %s" % (form, nrow, len(bad), bad[:5]))
    assert len(bad) == 0
    prob = run(image, 0, 3)
    excess = OG.softprob_excess_ulp(prob, OG.softprob_reference(margins))
    print("%s: softprob within %.2f ulp" % (form, excess.max()))
    assert np.all(excess <= 8)
    assert np.all(np.abs(prob.astype(np.float64).sum(axis=1) - 1.0) <= 1e-6)
    if form == "device":
        assert bits_equal(prob, predict_host(image, rows, NAN, 0))
    softmax = OG.multi_json(image, info, 3, "multi:softmax")
    cls = run(softmax, 0, 1)
    assert np.array_equal(cls[:, 0], np.argmax(margins, axis=1).astype(np.float32))
    assert len(np.unique(cls[ONE_TRIP:])) == 3


@pytest.mark.parametrize("ntree_limit", [0, 1])
def test_leaf_ids_past_one_trip(torch_cuda, big, ntree_limit):
    """nrow * L elements through group_leaf_gather: all T = 6 trees, and ntree_limit 1 (L = 3 < T: r = i / L, not i / T)."""
    image, trees, info, rows, _ = big
    nrow = len(rows)
    cnt, L = OG.group_counts(info, 3, ntree_limit)
    assert L == (6 if ntree_limit == 0 else 3) and nrow * L >= 2 * ONE_TRIP
    got = predict_host(image, rows, NAN, 16, ntree_limit)
    assert got.shape == (nrow, L)
    for g in range(3):
        cols = [t for t in range(L) if info[t] == g]
        sub = predict_host(OG.sub_json(image, info, g), rows, NAN, 16, cnt[g]).reshape(nrow, cnt[g])
        assert np.array_equal(got[:, cols], sub), g
    dev = predict_device(torch_cuda, image, rows, NAN, 16, ntree_limit, width=L)
    assert bits_equal(dev.reshape(nrow, L), got)


def shallow_contribs_booster(seed, G):
    """Small, shallow trees with consistent covers (the scatter does not care about a tree's shape; the depth-30 paths
    belong to test_gpu_contribs.py): -> (image, trees, tree_info)."""
    rng = np.random.default_rng(seed)
    thresholds = S.Thresholds(rng)
    trees = []
    for kind in ("small", "stump", "leaf", "small", "stump", "small"):
        t = S.make_tree(rng, kind, thresholds)
        S._consistent_covers(rng, t, False)
        trees.append(t)
    info = [t % G for t in range(len(trees))]
    return OG.multi_json(S.booster_json(trees, np.float32(0.25)), info, G), trees, info


@pytest.mark.parametrize("approximate", [False, True])
def test_contributions_past_one_trip(torch_cuda, approximate):
    G, nrow = 2, 2 * ONE_TRIP // 28 + 51
    assert nrow * 28 >= 2 * ONE_TRIP
    image, trees, info = shallow_contribs_booster(61, G)
    rows = many_rows(5, trees, nrow)
    b = booster(image)
    got = b.predict_contribs(capi.DMatrix(rows, missing=NAN), approximate=approximate)
    assert got.shape == (nrow, G, 28)
    for g in range(G):
        want = booster(OG.sub_json(image, info, g)).predict_contribs(capi.DMatrix(rows, missing=NAN), approximate=approximate)
        bad = np.nonzero((helpers.bits(got[:, g]) != helpers.bits(want)).any(axis=1))[0]
        print("group %d: %d of %d rows differ, the first %s" % (g, len(bad), nrow, bad[:5]))
        assert len(bad) == 0
    t = torch_cuda.from_numpy(rows).cuda()
    out = torch_cuda.full((nrow * G * 28,), NAN, dtype=torch_cuda.float32, device="cuda")
    d = capi.DMatrix(device_ptr=t.data_ptr(), nrow=nrow, ncol=27, missing=NAN)
    b.predict_contribs_device(d, out.data_ptr(), approximate=approximate)
    torch_cuda.cuda.synchronize()
    b.check()
    assert bits_equal(out.cpu().numpy().reshape(nrow, G, 28), got)


@pytest.mark.parametrize("approximate", [False, True])
def test_interactions_past_one_trip(approximate):
    G, nrow = 2, 2 * ONE_TRIP // 784 + 13
    assert nrow * 784 >= 2 * ONE_TRIP
    image, trees, info = shallow_contribs_booster(62, G)
    rows = many_rows(6, trees, nrow)
    got = booster(image).predict_interactions(capi.DMatrix(rows, missing=NAN), approximate=approximate)
    assert got.shape == (nrow, G, 28, 28)
    for g in range(G):
        want = booster(OG.sub_json(image, info, g)).predict_interactions(capi.DMatrix(rows, missing=NAN),
                                                                         approximate=approximate)
        assert bits_equal(got[:, g], want), g


# ---------------------------------------------------------------- group shapes

def check_against_the_parts(torch, image, info, G, rows, ntree_limit, contribs=True):
    nrow = len(rows)
    cnt, L = OG.group_counts(info, G, ntree_limit)
    want = expected_margins(image, info, G, rows, NAN, ntree_limit)
    got = predict_host(image, rows, NAN, 1, ntree_limit)
    assert got.shape == (nrow, G) and bits_equal(got, want)
    assert bits_equal(predict_device(torch, image, rows, NAN, 1, ntree_limit, width=G).reshape(nrow, G), want)
    base = OG.base_margin(image)
    for g in range(G):
        if cnt[g] == 0:
            assert bits_equal(got[:, g], np.full(nrow, base, np.float32))
    leaves = predict_host(image, rows, NAN, 16, ntree_limit)
    assert leaves.shape == (nrow, L)
    assert bits_equal(predict_device(torch, image, rows, NAN, 16, ntree_limit, width=L).reshape(nrow, L), leaves)
    for g in range(G):
        cols = [t for t in range(L) if info[t] == g]
        if cols:
            sub = predict_host(OG.sub_json(image, info, g), rows, NAN, 16, cnt[g]).reshape(nrow, cnt[g])
            assert np.array_equal(leaves[:, cols], sub), g
    if not contribs:
        return cnt
    for approximate in (False, True):
        phi = booster(image).predict_contribs(capi.DMatrix(rows, missing=NAN), approximate=approximate,
                                              ntree_limit=ntree_limit)
        assert phi.shape == (nrow, G, 28)
        for g in range(G):
            if cnt[g] == 0:
                assert np.all(phi[:, g, :27] == 0) and bits_equal(phi[:, g, 27], np.full(nrow, base, np.float32)), g
                continue
            sub = booster(OG.sub_json(image, info, g)).predict_contribs(capi.DMatrix(rows, missing=NAN),
                                                                        approximate=approximate, ntree_limit=cnt[g])
            assert bits_equal(phi[:, g], sub), (g, approximate)
    return cnt


@pytest.mark.parametrize("pattern", ["round_robin", "blocked"])
@pytest.mark.parametrize("ntree_limit", [0, 1, 2])
def test_two_groups(torch_cuda, pattern, ntree_limit):
    """G = 2; blocked with ntree_limit 1 or 2 leaves group 1 without a tree in the range (its plane is the memset)."""
    image, trees, info = OG.make_multi(5252, 10, 2, pattern, contribs=True)
    rows = S.rows_for(2, trees, 777, NAN)
    cnt = check_against_the_parts(torch_cuda, image, info, 2, rows, ntree_limit)
    if pattern == "blocked" and ntree_limit:
        assert cnt[1] == 0 and cnt[0] > 0


@pytest.mark.parametrize("ntree_limit", [1, 2])
def test_groups_emptied_by_ntree_limit(torch_cuda, ntree_limit):
    """G = 3, 12 trees in blocks: trees 0-3 are group 0's, 4-7 group 1's, 8-11 group 2's, so the first 3 or 6
    file trees leave group 2 (and, of 3, group 1) without a tree: their planes are the memset."""
    image, trees, info = OG.make_multi(5353, 12, 3, "blocked", contribs=True)
    rows = S.rows_for(3, trees, 600, NAN)
    cnt = check_against_the_parts(torch_cuda, image, info, 3, rows, ntree_limit)
    assert cnt[2] == 0 and cnt[0] > 0 and (cnt[1] > 0) == (ntree_limit > 1)


def test_64_groups_of_10_trees_and_a_group_that_is_one_root_leaf(torch_cuda):
    """Most groups are empty (the base margin), and group 40's only tree is a root leaf: base + that leaf in every row."""
    image, trees = S.contribs_booster(5454, 10)
    kinds = S.SMALL_PLANS[10]
    info = [63, 0, 17, 40, 5, 63, 17, 0, 31, 62]
    assert kinds[3] == "leaf" and len(trees[3].left) == 1 and info.count(40) == 1
    multi = OG.multi_json(image, info, 64)
    rows = S.rows_for(4, trees, 500, NAN)
    cnt = check_against_the_parts(torch_cuda, multi, info, 64, rows, 0)
    assert sum(1 for c in cnt if c == 0) == 64 - len(set(info))
    got = predict_host(multi, rows, NAN, 1)
    leaf = (OG.base_margin(multi) + np.float32(trees[3].cond[0])).astype(np.float32)
    assert bits_equal(got[:, 40], np.full(500, leaf, np.float32))
    prob = predict_host(multi, rows, NAN, 0)
    assert prob.shape == (500, 64)
    assert np.all(OG.softprob_excess_ulp(prob, OG.softprob_reference(got)) <= 8)
    # more groups than trees, and an ntree_limit: [0, min(T, k * G)) is all of them
    check_against_the_parts(torch_cuda, multi, info, 64, rows, 1, contribs=False)


# ---------------------------------------------------------------- the transforms on engineered margins

def device_form(torch, image, rows, option_mask, width):
    return predict_device(torch, image, rows, NAN, option_mask, width=width).reshape(len(rows), width)


@pytest.mark.parametrize("diff", OG.DIFFERENCES, ids=[str(d) for d in OG.DIFFERENCES])
@pytest.mark.parametrize("G", [2, 3, 5, 64])
def test_transforms_on_engineered_margins(torch_cuda, G, diff):
    """Boosters of root leaves and one stump: the margins are base + leaf (+ leaf) in float32, restated in numpy.
    Softprob against 1.6.0's formula in float64 from the FLOAT32 difference m_g - max (output_groups_support.py
    softprob_reference), within the project's 8 float32 ulp by np.spacing - 8 * 2**-149 in the denormal range, which a
    device that flushed denormal results of expf or of the division would break.  Softmax: np.argmax of the returned
    margins, the first maximum.  The device form gives the host form's bits."""
    rows = OG.engineered_rows()
    worst = 0.0
    for top in (0, G - 1):
        image, leaves, step = OG.engineered_booster(G, diff, top)
        want = OG.engineered_margins(leaves, step, rows)
        margins = predict_host(image, rows, NAN, 1)
        assert margins.shape == (len(rows), G)
        assert bits_equal(margins, want), (G, diff, top)
        assert bits_equal(device_form(torch_cuda, image, rows, 1, G), want)
        if diff == "signed_zero":
            assert np.all(margins == 0) and {bool(x) for x in np.signbit(margins).ravel()} == {True, False}
        prob = predict_host(image, rows, NAN, 0)
        assert prob.shape == (len(rows), G)
        ref = OG.softprob_reference(margins)
        excess = OG.softprob_excess_ulp(prob, ref)
        worst = max(worst, float(excess.max()))
        r, g = np.unravel_index(np.argmax(excess), excess.shape)
        print("G %d diff %s top %d: softprob within %.3f ulp (row %d group %d: %r against %r)" %
              (G, diff, top, excess.max(), r, g, float(prob[r, g]), float(ref[r, g])))
        assert np.all(excess <= 8), (G, diff, top, float(excess.max()))
        assert np.all(np.abs(prob.astype(np.float64).sum(axis=1) - 1.0) <= 1e-6)
        assert bits_equal(device_form(torch_cuda, image, rows, 0, G), prob)
        softmax, _, _ = OG.engineered_booster(G, diff, top, objective="multi:softmax")
        cls = predict_host(softmax, rows, NAN, 0)
        assert cls.shape == (len(rows),)
        assert np.array_equal(cls, np.argmax(margins, axis=1).astype(np.float32)), (G, diff, top)
        assert bits_equal(device_form(torch_cuda, softmax, rows, 0, 1)[:, 0], cls)
        target, _, _ = OG.engineered_booster(G, diff, top, objective="reg:squarederror", multi_target=True)
        value = predict_host(target, rows, NAN, 0)
        assert bits_equal(value, want)
        assert bits_equal(device_form(torch_cuda, target, rows, 0, G), want)
    print("G %d diff %s: worst %.3f ulp" % (G, diff, worst))


def test_the_first_maximum_wins_wherever_the_tie_stands(torch_cuda):
    """All groups equal: class 0.  G = 2 and 3, the last group below group 0 and lifted to an exact tie with it: still 0.
    Lifted past every group: G - 1; not lifted, the first of the groups that hold the largest leaf."""
    rows = OG.engineered_rows()
    lifted = rows[:, 0] >= 0
    assert lifted.any() and (~lifted).any()
    for G in (2, 3, 5, 64):
        image, leaves, step = OG.engineered_booster(G, "0", objective="multi:softmax")
        assert np.all(predict_host(image, rows, NAN, 0) == 0)
        image, leaves, step = OG.engineered_booster(G, 10.0, top=0, objective="multi:softmax")
        cls = predict_host(image, rows, NAN, 0)
        want = OG.engineered_margins(leaves, step, rows)
        assert np.array_equal(cls, np.argmax(want, axis=1).astype(np.float32))
        if G <= 3:
            assert leaves[G - 1] < leaves[0] and np.all(want[lifted, G - 1] == want[lifted, 0])
            assert np.all(cls == 0)                                         # tied with group 0, which stands first
        image, leaves, step = OG.engineered_booster(G, 10.0, top=G - 1, objective="multi:softmax")
        cls = predict_host(image, rows, NAN, 0)
        assert np.all(cls[lifted] == G - 1)                                 # past every other group
        assert np.all(cls[~lifted] == int(np.argmax(leaves)))
