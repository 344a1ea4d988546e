"""Node visit counts and the cover refresh, what can be checked without a GPU: the five entry points are declared,
bound and exported; every refusal that needs no device; leaf counters to node sums, the refresh arithmetic and the
launch plan through libohx_synth.so (the same functions of csrc/visits.cpp the product runs); and the kernels
cross-compile for gfx950 with no scratch and no flat memory instructions."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import categorical_support as CS
from tests import helpers
from tests import output_groups_support as OG
from tests import visits_support as V

HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["OHXBoosterCountVisits", "OHXBoosterCountVisitsDevice", "OHXBoosterGetVisitCounts",
           "OHXBoosterResetVisitCounts", "OHXBoosterRefreshCover"]
KERNELS = ["visits_lds_kernelILb1E", "visits_lds_kernelILb0E", "visits_global_kernelILb1E", "visits_global_kernelILb0E"]


def call(b, name):
    """The entry point with every argument after the handle NULL / 0 -> (rc, message)."""
    fn = getattr(b.lib, name)
    args = [b.handle]
    for t in fn.argtypes[1:]:
        args.append(0.0 if t is C.c_float else None)
    rc = fn(*args)
    return rc, b.lib.XGBGetLastError().decode()


def test_entry_points_declared_bound_and_exported():
    lib = C.CDLL(helpers.PRODUCT_SO)
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    f90 = open(os.path.join(helpers.ROOT, "quickchem_amd", "fortran", "ohx_bindings.F90")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert f'bind(C, name="{name}")' in f90, name
    for method in ("count_visits", "count_visits_device", "visit_counts", "reset_visit_counts", "refresh_cover"):
        assert hasattr(capi.Booster, method)
    # interface blocks only: the oracle-linked drivers link ohx_bindings.o and have no such symbols to resolve
    obj = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "obj", "ohx_bindings.o")
    nm = subprocess.run(["nm", "--undefined-only", obj], stdout=subprocess.PIPE, text=True).stdout
    assert "Visit" not in nm and "RefreshCover" not in nm


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    for phrase in ("ACCUMULATE", "\"ohx_device\" move", "no float atomics", "prior_weight * sum_hess_old",
                   "no fused multiply-add", "not capturable", "OHXReleaseScratch leaves it alone"):
        assert phrase in header, phrase


@pytest.mark.parametrize("name", SYMBOLS)
def test_no_model_is_refused(name):
    b = capi.Booster()
    rc, msg = call(b, name)
    assert rc == -1 and "holds no model" in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
def test_a_categorical_booster_is_refused_at_the_top(name):
    js, _, _ = CS.make_booster(5, 3)
    b = capi.Booster(model_buffer=js)
    rc, msg = call(b, name)
    assert rc == -1 and "categorical" in msg and name in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
def test_several_output_groups_are_refused_at_the_top(name):
    js, _, _ = OG.make_multi(8, 6, 3, "round_robin")
    b = capi.Booster(model_buffer=js)
    rc, msg = call(b, name)
    assert rc == -1 and "single-output" in msg and "3 output groups" in msg, msg


def test_null_arguments_and_bad_prior_weights_are_refused():
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    rc, msg = call(b, "OHXBoosterGetVisitCounts")
    assert rc == -1 and "NULL output argument" in msg, msg
    for name in ("OHXBoosterCountVisits", "OHXBoosterCountVisitsDevice"):
        rc, msg = call(b, name)                       # a NULL matrix
        assert rc == -1 and "DMatrix handle is invalid" in msg, msg
    for w in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(capi.OhxError, match="prior_weight must be finite and >= 0"):
            b.refresh_cover(w)
    with pytest.raises(capi.OhxError, match="no row has been counted yet"):
        b.refresh_cover(0.0)
    with pytest.raises(capi.OhxError, match="no row has been counted yet"):
        b.refresh_cover(0.5)


def test_the_knobs_reject_what_they_do_not_know():
    b = capi.Booster()
    for value in ("LDS", "", "0"):
        with pytest.raises(capi.OhxError, match="ohx_visits_kernel must be auto, global or lds"):
            b.set_param("ohx_visits_kernel", value)
    for value in ("eight", "8 leaves", "", "-1", "1e3", "4294967296"):
        with pytest.raises(capi.OhxError, match="ohx_visits_lds_leaves must be auto or a whole number"):
            b.set_param("ohx_visits_lds_leaves", value)
    for value in ("auto", "0", "1", "8", "2147483647"):
        b.set_param("ohx_visits_lds_leaves", value)
    for value in ("auto", "global", "lds"):
        b.set_param("ohx_visits_kernel", value)


def test_before_any_count_everything_is_zero_and_reset_is_harmless():
    js, _ = S.make_booster(12, 5)
    trees = V.doc_trees(js)
    b = capi.Booster(model_buffer=js)
    for _ in range(2):
        counts, seen = b.visit_counts()
        assert seen == 0 and [len(c) for c in counts] == [len(t["left_children"]) for t in trees]
        assert all(not c.any() for c in counts)
        V.check_invariants(trees, counts, 0)
        b.reset_visit_counts()


# ---- leaf counters to node sums ----

def test_the_layout_numbers_leaves_in_file_order():
    js, leaves = V.hand_booster()
    offs, loff, lnode = synth.visits_layout(js)
    assert offs.tolist() == [0, 1, 4, 11, 16]
    assert loff.tolist() == [0, 1, 3, 7, 9]
    assert lnode.tolist() == [n for t in leaves for n in t]


def test_node_sums_on_hand_made_trees():
    """A root leaf, a stump, a chain, and a tree with deleted slots."""
    js, leaves = V.hand_booster()
    trees = V.doc_trees(js)
    leaf_counts = np.array([13, 4, 9, 6, 0, 5, 2, 1 << 40, 3], dtype=np.uint64)
    got = synth.visits_node_sums(js, leaf_counts)
    offs = synth.visits_layout(js)[0]
    per_tree = [got[int(offs[t]):int(offs[t + 1])] for t in range(4)]
    assert per_tree[0].tolist() == [13]
    assert per_tree[1].tolist() == [13, 4, 9]
    assert per_tree[2].tolist() == [13, 6, 7, 0, 7, 5, 2]
    assert per_tree[3].tolist() == [(1 << 40) + 3, 0, 0, 1 << 40, 3]       # deleted slots 1 and 2 stay 0
    # ... and the tests' own sum agrees
    k = 0
    for t, tree in enumerate(trees):
        at_leaves = np.zeros(len(tree["left_children"]), dtype=np.uint64)
        for n in leaves[t]:
            at_leaves[n] = leaf_counts[k]
            k += 1
        assert np.array_equal(per_tree[t], V.sum_up(tree, at_leaves))


def test_node_sums_on_adversarial_boosters():
    js, _ = S.make_booster(21, 10)
    trees = V.doc_trees(js)
    offs, loff, lnode = synth.visits_layout(js)
    rng = np.random.default_rng(3)
    leaf_counts = rng.integers(0, 1000, int(loff[-1])).astype(np.uint64)
    leaf_counts[rng.random(leaf_counts.size) < 0.4] = 0
    got = synth.visits_node_sums(js, leaf_counts)
    for t, tree in enumerate(trees):
        assert [n for n in range(len(tree["left_children"])) if tree["left_children"][n] == -1] == \
            lnode[int(loff[t]):int(loff[t + 1])].tolist()
        at_leaves = np.zeros(len(tree["left_children"]), dtype=np.uint64)
        at_leaves[lnode[int(loff[t]):int(loff[t + 1])]] = leaf_counts[int(loff[t]):int(loff[t + 1])]
        assert np.array_equal(got[int(offs[t]):int(offs[t + 1])], V.sum_up(tree, at_leaves)), t


# ---- the refresh arithmetic ----

def _node_counts(js, seed, zero=0.0, big=False):
    """Consistent node counts from random leaf counts -> (flat uint64, per tree)."""
    trees = V.doc_trees(js)
    offs, loff, lnode = synth.visits_layout(js)
    rng = np.random.default_rng(seed)
    leaf_counts = rng.integers(1, (1 << 33) if big else 8, int(loff[-1])).astype(np.uint64)
    leaf_counts[rng.random(leaf_counts.size) < zero] = 0
    flat = synth.visits_node_sums(js, leaf_counts)
    return flat, [flat[int(offs[t]):int(offs[t + 1])] for t in range(len(trees))]


@pytest.mark.parametrize("prior_weight", [0.0, 1.0, 1e-3])
@pytest.mark.parametrize("big", [False, True], ids=["small counts", "counts past 2^24"])
def test_the_refresh_is_numpy_float32(prior_weight, big):
    js, _ = S.contribs_booster(31, 10)
    trees = V.doc_trees(js)
    flat, per_tree = _node_counts(js, 7, big=big)
    got, err = synth.visits_refresh(js, flat, prior_weight)
    assert err is None, err
    want = np.concatenate([V.expected_cover(t, c, prior_weight) for t, c in zip(trees, per_tree)])
    assert np.array_equal(helpers.bits(got), helpers.bits(want))
    if prior_weight == 1e-3 and not big:
        # the set tells a fused multiply-add (one rounding) from the product rounded and then the sum
        fused = np.concatenate([(c.astype(np.float32).astype(np.float64) + np.float64(np.float32(prior_weight)) *
                                 np.asarray(t["sum_hessian"], np.float32).astype(np.float64)).astype(np.float32)
                                for t, c in zip(trees, per_tree)])
        assert np.any(helpers.bits(fused) != helpers.bits(want))


def test_unreachable_and_deleted_slots_keep_their_cover():
    js, _ = V.hand_booster()
    trees = V.doc_trees(js)
    flat = synth.visits_node_sums(js, np.array([5, 2, 3, 1, 1, 1, 2, 4, 1], dtype=np.uint64))
    got, err = synth.visits_refresh(js, flat, 0.0)
    assert err is None, err
    offs = synth.visits_layout(js)[0]
    last = got[int(offs[3]):]
    assert last.tolist() == [5.0, 77.0, 88.0, 4.0, 1.0]
    assert np.array_equal(got, np.concatenate([V.expected_cover(t, flat[int(offs[i]):int(offs[i + 1])], 0.0)
                                               for i, t in enumerate(trees)]))


def test_a_zero_count_split_is_refused_by_name_and_a_zero_count_leaf_is_not():
    js, _ = V.hand_booster()
    trees = V.doc_trees(js)
    old = np.concatenate([np.asarray(t["sum_hessian"], np.float32) for t in trees])
    # tree 2 (the chain): nothing reaches node 2, so the splits at nodes 2 and 4 get count 0; tree 1's leaf 2 too
    flat = synth.visits_node_sums(js, np.array([6, 6, 0, 6, 0, 0, 0, 2, 4], dtype=np.uint64))
    got, err = synth.visits_refresh(js, flat, 0.0)
    assert err is not None and "node 2 of tree 2" in err and "2 of 5 splits" in err and "prior_weight" in err, err
    assert np.array_equal(helpers.bits(got), helpers.bits(old)), "a refused refresh changed the forest"
    # blended with the old cover the same counts pass, and the leaf of old cover 0 keeps 0
    got, err = synth.visits_refresh(js, flat, 1e-3)
    assert err is None, err
    offs = synth.visits_layout(js)[0]
    chain = got[int(offs[2]):int(offs[3])]
    assert np.all(np.isfinite(got)) and chain[2] == np.float32(1e-3) * np.float32(6.0) and chain[5] == 0.0
    # a zero-count LEAF beside a counted one is legal with prior_weight 0
    flat = synth.visits_node_sums(js, np.array([6, 6, 0, 1, 1, 2, 2, 2, 4], dtype=np.uint64))
    got, err = synth.visits_refresh(js, flat, 0.0)
    assert err is None and got[int(offs[1]) + 2] == 0.0, err


def test_a_cover_that_overflows_float32_is_refused():
    js, _ = V.hand_booster()
    flat = synth.visits_node_sums(js, np.array([6, 3, 3, 1, 1, 2, 2, 2, 4], dtype=np.uint64))
    got, err = synth.visits_refresh(js, flat, 3e38)
    assert err is not None and "node 0 of tree 1" in err, err


# ---- the launch plan ----

def test_the_plan_at_several_capacities():
    js, _ = S.make_booster(41, 10)
    trees = V.doc_trees(js)
    leaves = np.array([sum(1 for x in V.reachable(t) if t["left_children"][x] == -1) for t in trees])
    tiles = 4 * 27 * 64 * 4
    p = synth.visits_plan(js)
    assert p["stage"] and p["capacity"] == (160 * 1024 - tiles) // 4
    assert p["takes_lds"].all() and p["hist_leaves"] == leaves.max()
    assert p["lds_bytes_lds"] == tiles + 4 * leaves.max() and p["lds_bytes_global"] == tiles
    for cap in (1, 8, int(np.sort(leaves)[len(leaves) // 2]), int(leaves.max()) - 1, int(leaves.max())):
        p = synth.visits_plan(js, lds_leaves=cap)
        assert np.array_equal(p["takes_lds"], leaves <= cap), cap
        assert p["hist_leaves"] == leaves[leaves <= cap].max(initial=0)
        assert p["lds_bytes_lds"] <= 160 * 1024
    assert 0 < synth.visits_plan(js, lds_leaves=8)["lds_trees"] < len(trees), "8 mixes both ways in this booster"
    p = synth.visits_plan(js, force_global=True)
    assert not p["takes_lds"].any() and p["hist_leaves"] == 0
    # blocks: one trip of the LDS kernel's loop is CUs x 256 rows per tree, of the global kernel's four times that
    p = synth.visits_plan(js, num_cus=256, ntiles=1 << 20)
    assert p["lds_blocks"] == 256 * capi.VISITS_LDS_BLOCKS_PER_CU and p["global_blocks"] == 256 * capi.VISITS_GLOBAL_BLOCKS_PER_CU
    p = synth.visits_plan(js, num_cus=256, ntiles=5)
    assert p["lds_blocks"] == 2 and p["global_blocks"] == 2
    assert capi.VISITS_BLOCK_ROWS == 256


@pytest.mark.parametrize("nfeat,stage", [(1, True), (27, True), (100, True), (128, True), (129, False), (300, False)])
def test_rows_are_staged_only_where_a_blocks_tiles_fit(nfeat, stage):
    js = V.random_booster(50 + nfeat, 3, nfeat, max_depth=4)
    p = synth.visits_plan(js)
    assert p["stage"] == stage
    tiles = 4 * nfeat * 64 * 4 if stage else 0
    assert p["lds_bytes_global"] == tiles and p["capacity"] == (160 * 1024 - tiles) // 4 and p["capacity"] >= 8192
    assert p["lds_bytes_lds"] <= 160 * 1024


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "visits.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "visits.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel_body(text, name_part):
    m = re.search(r"^(_Z\w*" + re.escape(name_part) + r"\w*):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, name_part
    return m.group(2)


@pytest.mark.parametrize("kernel", KERNELS)
def test_visit_kernels_have_no_scratch_no_flat_access_and_no_float_atomics(isa, kernel):
    body = kernel_body(isa, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add", body), "a float atomic"
    assert "global_atomic_add_x2" in body, "the counters are added to with 64-bit integer adds"
    assert "cmpswap" not in body
    if "lds_kernel" in kernel:
        assert "ds_add_u32" in body, "the histogram is counted with LDS atomics"
