"""Boosting with row and column subsampling, what can be checked without a GPU: the two entry points are declared, bound,
exported and placed; the header states the semantics; every refusal that needs no device, with outputs and saved bytes
unchanged; the bag and the selected features from the host build of the shared functions against the restatement
(tests/grow_sampled_support.py); n_sel and the tie rule; the quality of the bag; the plan over n_sel features; the new
kernels cross-compile for gfx950 with no scratch, no flat access, no float atomic and no compare-and-swap; the host
functions under sanitizers in a program of their own; and the restatement on a case worked by hand."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_sampled_support as P
from tests import grow_weighted_support as W
from tests import helpers
from tests.test_grow_cpu import _hand_tree, kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["OHXBoosterBoostTreesSampled", "OHXBoosterBoostTreesSampledDevice"]
KERNELS = ["grow_bag_kernel", "grow_hist_sampled_kernel", "grow_split_sampled_kernelILi0E", "grow_split_sampled_kernelILi1E"]
SENTINEL = 12345
Q = 1 << 24
SEEDS = (0, 1, 42, (1 << 63) + 5)
TREES = (0, 1, 2, 3, (1 << 32) + 7)
NAN = float("nan")


def call(b, name, dmat=None, labels=True, nfeat=3, rounds=2, max_depth=3, eta=0.3, lam=1.0, gamma=0.0, min_child_weight=1.0,
         subsample=1.0, colsample=1.0, seed=0, patience=0, cut_ptr=True, descending_cuts=False):
    """-> (rc, message); asserts that a refused call wrote no output."""
    y = np.zeros(4, dtype=np.float32)
    ptr, vals = np.arange(nfeat + 1, dtype=np.uint64), np.arange(nfeat, dtype=np.float32)
    if descending_cuts:
        ptr = ptr[::-1].copy()
    train = np.full(rounds + 1 if rounds > 0 else 1, -7.0)
    held = train.copy()
    r, k, n = C.c_int32(SENTINEL), C.c_int32(SENTINEL), C.c_uint64(SENTINEL)
    args = [b.handle, dmat, y.ctypes.data if labels else None, None, 4, None, None, None, 0,
            ptr.ctypes.data if cut_ptr else None, vals.ctypes.data, rounds, max_depth, eta, lam, gamma, min_child_weight,
            subsample, colsample, seed, patience, train.ctypes.data, held.ctypes.data, C.byref(r), C.byref(k), C.byref(n)]
    if name.endswith("Device"):
        args.append(None)
    rc = getattr(b.lib, name)(*args)
    if rc != 0:
        assert (r.value, k.value, n.value) == (SENTINEL,) * 3, "a refused call wrote an output"
        assert np.all(train == -7.0) and np.all(held == -7.0), "a refused call wrote an RMSE"
    return rc, b.lib.XGBGetLastError().decode()


def test_entry_points_declared_bound_exported_and_placed():
    lib = C.CDLL(helpers.PRODUCT_SO)
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    f90 = open(os.path.join(helpers.ROOT, "quickchem_amd", "fortran", "ohx_bindings.F90")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert re.search(r" T " + name + r"$", nm, re.M), name
        assert f'bind(C, name="{name}")' in f90, name
        assert header.index("int OHXBoosterBoostTreesWeightedDevice(") < header.index("int " + name + "(") < header.index("int OHXQuantileCuts(")
        assert f90.index('name="OHXBoosterBoostTreesWeightedDevice"') < f90.index(f'name="{name}"') < f90.index('name="OHXQuantileCuts"')
        # three more arguments before patience
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S).group(1)
        assert re.search(r"float min_child_weight,\s*float subsample,\s*float colsample_bytree,\s*uint64_t seed,\s*int patience", decl), name
    for method in ("boost_trees_sampled", "boost_trees_sampled_device"):
        assert hasattr(capi.Booster, method)
    for f in ("boost_bag", "boost_features", "grow_plan_sampled"):
        assert hasattr(synth, f)
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.SYNTH_SO], stdout=subprocess.PIPE, text=True).stdout
    for f in ("ohx_grow_bag", "ohx_grow_features", "ohx_grow_plan_sampled"):
        assert re.search(r" T " + f + r"$", nm, re.M), f


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    header = re.sub(r"\s*\n \*\s*", " ", header)          # comment lines joined
    for phrase in ("mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31",
                   "All arithmetic is uint64 and wraps", "gamma64 = 0x9E3779B97F4A7C15", "i = T0 + t - 1",
                   "number of trees the forest holds when the call starts", "K_row(i) = mix(seed + gamma64 * (2i + 1))",
                   "K_col(i) = mix(seed + gamma64 * (2i + 2))", "k_s = (uint32) rint((double)subsample * 2^24)",
                   "(mix(K_row(i) + r) >> 40) < k_s", "puts every row in and draws nothing",
                   "n_sel = max(1, (int) floor((double)colsample_bytree * F))", "c_f = mix(K_col(i) + f)",
                   "smallest by (c_f, f), kept in ascending f", "n_sel == F selects all and draws nothing",
                   "every out-of-bag row has weight 0", "every unselected feature has an empty cut list",
                   "sum_hess, base_weight and min_child_weight are over the bag", "with the original f",
                   "pred += leaf(row) for every row, in or out of the bag", "still refused with \"label\"",
                   "only through r in the draw", "Integer adds only",
                   "equal those of OHXBoosterBoostTreesWeighted", "after min_child_weight and before the cuts",
                   "or with k_s == 0", "root H == 0", "the message says \"bag\""):
        assert phrase in header, phrase


# ---- refusals that need no device ----

@pytest.mark.parametrize("name", SYMBOLS)
def test_bad_arguments_are_refused_before_a_matrix_is_looked_at(name):
    js, _ = S.make_booster(11, 3)
    import json
    F = int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])
    rc, msg = call(capi.Booster(), name)
    assert rc == -1 and "holds no model" in msg, msg
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    # what the Weighted call refuses, under this call's name
    rc, msg = call(b, name, nfeat=F, labels=False)
    assert rc == -1 and name in msg and "labels is NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, rounds=0)
    assert rc == -1 and "rounds must be >= 1" in msg, msg
    rc, msg = call(b, name, nfeat=F, min_child_weight=-1.0)
    assert rc == -1 and "min_child_weight must be finite and >= 0" in msg, msg
    rc, msg = call(b, name, nfeat=F, patience=-1)
    assert rc == -1 and "patience must be >= 0" in msg, msg
    # its own
    tiny = float(np.float32(2.0 ** -26))             # finite and > 0, but k_s == 0
    for bad in (NAN, float("inf"), float("-inf"), 0.0, -0.5, float(np.nextafter(np.float32(1), np.float32(2))), 2.0, tiny,
                float(np.float32(2.0 ** -25))):
        rc, msg = call(b, name, nfeat=F, subsample=bad)
        assert rc == -1 and name in msg and "subsample must be finite, > 0 and <= 1" in msg, (bad, msg)
    for bad in (NAN, float("inf"), float("-inf"), 0.0, -0.5, float(np.nextafter(np.float32(1), np.float32(2))), 2.0):
        rc, msg = call(b, name, nfeat=F, colsample=bad)
        assert rc == -1 and name in msg and "colsample_bytree must be finite, > 0 and <= 1" in msg, (bad, msg)
    # the order: min_child_weight, subsample, colsample_bytree, the cuts, patience
    rc, msg = call(b, name, nfeat=F, min_child_weight=-1.0, subsample=0.0)
    assert rc == -1 and "min_child_weight" in msg, msg
    rc, msg = call(b, name, nfeat=F, subsample=0.0, colsample=0.0)
    assert rc == -1 and "subsample must be" in msg, msg
    rc, msg = call(b, name, nfeat=F, colsample=0.0, descending_cuts=True)
    assert rc == -1 and "colsample_bytree" in msg, msg
    rc, msg = call(b, name, nfeat=F, subsample=0.0, patience=-1)
    assert rc == -1 and "subsample" in msg, msg
    rc, msg = call(b, name, nfeat=F, descending_cuts=True, patience=-1)
    assert rc == -1 and "patience" not in msg and "subsample" not in msg, msg
    # every argument sound (the smallest subsample and colsample, any seed): the NULL matrix is what is left
    for kw in ({}, {"subsample": 2.0 ** -24, "colsample": 2.0 ** -20, "seed": (1 << 64) - 1}, {"subsample": 0.5, "colsample": 0.5}):
        rc, msg = call(b, name, nfeat=F, **kw)
        assert rc == -1 and "DMatrix handle is invalid" in msg, msg
    assert saved(b) == before, "a refusal changed the forest"


# ---- the draws ----

def test_the_mix_function_is_the_finalizer_of_splitmix64():
    """The first outputs of SplitMix64 seeded with 0 (Steele, Lea and Flood; the values every implementation's test
    vectors list): the state advances by gamma64 and mix() finishes it."""
    known = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    with np.errstate(over="ignore"):
        assert [int(P.mix(P.GAMMA64 * np.uint64(k + 1))) for k in range(3)] == known
    assert int(P.row_key(0, 0)) == known[0] and int(P.col_key(0, 0)) == known[1] and int(P.row_key(0, 1)) == known[2]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_bag_against_the_restatement(seed):
    one = float(np.float32(1.0) - np.float32(2.0 ** -24))
    for tree in TREES:
        for n in (1, 63, 64, 65, 4097):
            for k_s, s in ((1, 2.0 ** -24), (1 << 23, 0.5), ((1 << 24) - 1, one), (1 << 24, 1.0)):
                got, ks = synth.boost_bag(seed, tree, n, s)
                assert ks == k_s == P.threshold(s)
                want = P.bag(seed, tree, n, s)
                assert got.dtype == bool and got.shape == (n,) and np.array_equal(got, want), (seed, tree, n, s)
                if k_s == 1 << 24:
                    assert got.all()
    # the tree index and the seed move the draw; a row's draw does not depend on nrow
    a = synth.boost_bag(seed, 0, 4097, 0.5)[0]
    assert not np.array_equal(a, synth.boost_bag(seed, 1, 4097, 0.5)[0])
    assert not np.array_equal(a, synth.boost_bag(seed + 1, 0, 4097, 0.5)[0])
    assert not np.array_equal(a, synth.boost_bag(seed, 1 << 32, 4097, 0.5)[0]), "a tree index past 2^32 is not cut to 32 bits"
    assert np.array_equal(a[:65], synth.boost_bag(seed, 0, 65, 0.5)[0])
    # a smaller threshold's bag lies inside a larger one's
    assert not (synth.boost_bag(seed, 0, 4097, 0.25)[0] & ~a).any()
    for bad in (0.0, -1.0, 1.5, NAN, 2.0 ** -26):
        with pytest.raises(capi.OhxError):
            synth.boost_bag(seed, 0, 8, bad)
        with pytest.raises(ValueError, match="^subsample"):
            P.threshold(bad)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_selected_features_against_the_restatement(seed):
    for tree in TREES:
        for F in (1, 3, 27, 128):
            for c in (2.0 ** -20, 0.01, 0.3, 0.34, 0.5, 0.67, 0.99, 1.0):
                got = synth.boost_features(seed, tree, F, c)
                want = P.features(seed, tree, F, c)
                assert got.dtype == np.uint8 and got.tolist() == want, (seed, tree, F, c)
                assert len(want) == P.num_selected(F, c) and want == sorted(set(want)) and want[-1] < F
    assert synth.boost_features(seed, 0, 27, 0.5).tolist() != synth.boost_features(seed, 1, 27, 0.5).tolist()
    assert synth.boost_features(seed, 0, 128, 0.5).tolist() != synth.boost_features(seed, 1 << 32, 128, 0.5).tolist()
    assert synth.boost_features(seed, 5, 27, 1.0).tolist() == list(range(27))
    for bad in (0.0, -1.0, 1.5, NAN):
        with pytest.raises(capi.OhxError):
            synth.boost_features(seed, 0, 27, bad)
        with pytest.raises(ValueError, match="^colsample"):
            P.num_selected(27, bad)


def test_n_sel():
    want = {(1, 2.0 ** -20): 1, (1, 0.5): 1, (1, 1.0): 1, (3, 2.0 ** -20): 1, (3, 0.33): 1, (3, 0.34): 1, (3, 0.67): 2,
            (3, 0.99): 2, (3, 1.0): 3, (27, 2.0 ** -20): 1, (27, 0.5): 13, (27, 0.3): 8, (27, 0.99): 26, (27, 1.0): 27,
            (128, 2.0 ** -20): 1, (128, 2.0 ** -7): 1, (128, 2.0 ** -6): 2, (128, 0.5): 64, (128, 0.3): 38, (128, 1.0): 128}
    for (F, c), n in want.items():
        assert P.num_selected(F, c) == n, (F, c)
        assert len(synth.boost_features(7, 0, F, c)) == n, (F, c)
        assert synth.grow_plan_sampled(4097, F, c, 0, 8, 256)["n_sel"] == n
    # (double)0.34f * 3 = 1.0200000107..., floor 1; (double)0.3f * 128 = 38.4000015..., floor 38
    assert float(np.float32(0.34)) * 3 > 1.02 and float(np.float32(0.3)) * 128 > 38.4


def test_key_ties_go_to_the_smaller_feature():
    """Forced by hand through (c_f, f): equal keys are taken in the order of the feature."""
    assert P.select([5, 5, 5, 5], 2) == [0, 1]
    assert P.select([9, 5, 5, 1], 2) == [1, 3]
    assert P.select([9, 5, 5, 1], 3) == [1, 2, 3]
    assert P.select([7, 7, 3, 7, 3], 3) == [0, 2, 4]
    assert P.select([(1 << 64) - 1, 0, (1 << 64) - 1], 2) == [0, 1]
    assert P.select([3, 2, 1], 3) == [0, 1, 2], "kept in ascending f"


def test_the_bag_fraction_at_a_million_rows():
    """2^20 rows at subsample 0.5: sigma = sqrt(0.25 / 2^20) = 0.000488, and 5 sigma = 0.0025 (rounded up)."""
    n = 1 << 20
    worst = 0.0
    for seed in SEEDS:
        for tree in (0, 1, 2, 3):
            got, _ = synth.boost_bag(seed, tree, n, 0.5)
            frac = float(got.mean())
            print(f"seed {seed} tree {tree}: bag fraction {frac:.6f}")
            worst = max(worst, abs(frac - 0.5))
            assert abs(frac - 0.5) <= 0.0025, (seed, tree, frac)
            if seed == 42 and tree == 3:
                assert np.array_equal(got, P.bag(seed, tree, n, 0.5))
    print(f"largest distance from 0.5: {worst:.6f}")


# ---- the plan ----

@pytest.mark.parametrize("nrow", [1, 4097, 55987200, 1 << 31])
def test_the_plan_over_the_selected_features(nrow):
    for n_sel in range(1, 129):
        for F, c in ((n_sel, 1.0), (128, n_sel / 128.0)):
            p = synth.grow_plan_sampled(nrow, F, c, 0, 8, 256)
            w = synth.grow_plan_weighted(nrow, n_sel, 0, 8, 256)
            assert p["n_sel"] == n_sel and p["levels"] == w["levels"] and p["hist_bytes"] == w["hist_bytes"]
            assert p["bins_bytes"] == F * nrow, "the bins hold every feature"
            assert p["row_blocks"] == w["row_blocks"] and p["max_pairs"] == 40 and p["pair_bytes"] == 256 * 16
            assert p["hist_bytes"] == 128 * n_sel * 256 * 16, "compact: [slots][n_sel][256]"
            for l in p["levels"]:
                assert l["node_group"] * l["feat_group"] <= 40 and l["lds_bytes"] <= 160 * 1024
                assert l["feat_groups"] * l["feat_group"] >= n_sel > (l["feat_groups"] - 1) * l["feat_group"]


def test_half_the_features_of_the_benchmark_shape():
    """C360 L72 with 27 features at colsample 0.5: 13 features in 13 groups at level 5, against 27."""
    p = synth.grow_plan_sampled(55987200, 27, 0.5, 6639, 6, 256)
    assert p["n_sel"] == 13
    assert [(l["node_group"], l["feat_group"], l["node_groups"], l["feat_groups"]) for l in p["levels"]] == [
        (1, 13, 1, 1), (2, 13, 1, 1), (4, 7, 1, 2), (8, 5, 1, 3), (16, 2, 1, 7), (32, 1, 1, 13)]


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_sampled.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_sampled.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read(), r.stderr


def _figure(report, kernel, what):
    m = re.search(r"Function Name: \S*" + re.escape(kernel) + r".*?" + re.escape(what) + r": (\d+)", report, re.S)
    assert m, (kernel, what)
    return int(m.group(1))


@pytest.mark.parametrize("kernel", KERNELS)
def test_sampled_kernels_resources_and_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    adds = len(re.findall(r"global_atomic_add_x2", body))
    if "hist" in kernel:
        assert len(re.findall(r"ds_add_u64", body)) >= 2 and "ds_add_u32" not in body, "both sums are 64-bit LDS integer adds"
        assert adds == 2, "flushed with 64-bit global integer adds, one a sum"
    else:
        assert "atomic_add" not in body and "ds_add" not in body
    if "bag" in kernel:
        assert len(re.findall(r"global_store_dwordx2", body)) == 1 and "global_load" not in body, "a word a wave, and nothing read"
        assert len(re.findall(r"v_mad_u64_u32|v_mul_hi_u32|v_mul_lo_u32", body)) >= 4, "the draw multiplies 64-bit integers twice"
    if "ILi0E" in kernel:
        assert "v_div_scale_f64" in body, "the gain divides in double"
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    lds = {"grow_bag_kernel": 0, "grow_hist_sampled_kernel": 0, "grow_split_sampled_kernelILi0E": 0,
           "grow_split_sampled_kernelILi1E": 256 * 4}[kernel]
    assert _figure(report, kernel, "LDS Size [bytes/block]") == lds, "static LDS (the histogram's is dynamic)"
    # registers: the streaming kernels keep 8 waves a SIMD (at most 64 VGPRs); the split kernels need at least 4
    vgprs, occupancy = _figure(report, kernel, "VGPRs"), _figure(report, kernel, "Occupancy [waves/SIMD]")
    if "split" in kernel:
        assert vgprs <= 128 and occupancy >= 4, (vgprs, occupancy)
    else:
        assert vgprs <= 64 and occupancy == 8, (vgprs, occupancy)


def test_the_kernel_files_hold_their_own_kernels():
    src = open(os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_sampled.hip")).read()
    assert sorted(set(re.findall(r"void (grow_\w+_kernel)\(", src))) == sorted(
        ["grow_bag_kernel", "grow_hist_sampled_kernel", "grow_split_sampled_kernel"])
    csrc = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    assert not os.path.exists(os.path.join(csrc, "grow_split_device.hpp")), "grow_device.hpp replaces it"
    # the split choice is one text for the plain, the weighted and the sampled kernels: the shared header holds both
    # phases, the only call of the scan among the device files, and no kernel
    shared = open(os.path.join(csrc, "grow_device.hpp")).read()
    assert shared.count("grow_best_split<") == 1 and "__global__" not in shared
    for what in ("void grow_level_range(", "GrowCand grow_shuffle_cand(", "void grow_write_leaf(", "void grow_split_columns(",
                 "void grow_split_nodes(", "hipError_t grow_launch_tree("):
        assert shared.count(what) == 1, what
    assert len(re.findall(r"for \(uint32_t d = 0; d < \(uint32_t\)a\.max_depth; \+\+d\)", shared)) == 1, "the one level loop"
    for name in ("grow.hip", "grow_weighted.hip", "grow_sampled.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "grow_device.hpp"' in text, name
        assert "grow_split_columns(" in text and "grow_split_nodes<" in text and "grow_launch_tree(" in text, name
        # no split scan, no prefix sums, no candidate shuffle, no leaf record and no level loop of its own
        for own in ("grow_best_split", "__shfl_up", "__shfl_xor(c.", "r.base_weight", "a.max_depth; ++d", "hipMemsetAsync"):
            assert own not in text, (name, own)
    hdr = open(os.path.join(csrc, "grow.hpp")).read()
    assert len(re.findall(r"GrowCand grow_best_split\(", hdr)) == 1 and "grow_best_split_weighted" not in hdr
    for gone in ("GrowWeightedArgs", "GrowSampledArgs", "GrowWeightedEvalArgs", "prepare_grow_weighted", "prepare_grow_sampled"):
        for name in sorted(os.listdir(csrc)):
            assert gone not in open(os.path.join(csrc, name), errors="replace").read(), (gone, name)
    for name in ("grow.hip", "grow_eval.hip", "grow_weighted.hip"):
        assert "sampled" not in open(os.path.join(csrc, name)).read(), name


# ---- the host functions under sanitizers ----

def test_the_host_functions_under_sanitizers(tmp_path):
    """tools/grow_sampled_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only): the keys with
    wrapping arguments, the threshold and n_sel at their edges, the features into a buffer of exactly n_sel bytes, the
    bag's fraction, and the plan over 1 to 128 selected features."""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_sampled_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_sampled_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe), "300", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


# ---- the restatement itself ----

def test_the_restatement_on_a_case_worked_by_hand():
    """The 8 rows of test_grow_cpu's hand case, unit weights, base 0, eta 1, lambda 0, depth 2, seed 0, subsample 0.5 and
    colsample 0.5 of two features.  Tree 0 of seed 0: K_row = 0xE220A8397B1DCDAF, the bag is rows 0, 3, 4, 5 and the one
    feature is f1.  g over the bag = 0, -2, -4, -4: G = -10, H = 4, gain 25.  f1: rows 0, 4 left (G = -4, H = 2: 8), rows
    3, 5 right (G = -6, H = 2: 18): loss_chg 1.  f0 would give 2 | 8 with H 2 | 2: 2 + 32 - 25 = 9, more - but it is
    not selected.  Both children hold one value of f1 each: leaves 4/2 = 2 and 6/2 = 3.  Every row moves: pred = 2 where
    f1 = 1, 3 where f1 = 2; pred - y = 2, 1, 2, 1, -2, -1, -2, -1, so S_1 = 20 * 2^72 over all eight rows and
    S_0 = 72 * 2^72, W = 8 * 2^24."""
    x, y, cuts = _hand_tree()
    z = np.zeros(8, np.float32)
    assert P.bag(0, 0, 8, 0.5).tolist() == [True, False, False, True, True, True, False, False]
    assert P.features(0, 0, 2, 0.5) == [1]
    kw = dict(rounds=1, max_depth=2, eta=1.0, lam=0.0, min_child_weight=0.0, subsample=0.5, colsample_bytree=0.5, seed=0)
    out = P.boost_sampled(z, x, NAN, y, None, cuts, 2, **kw)
    t = out["trees"][0]
    lb = -(1 << 31)
    assert t["left"].tolist() == [1, -1, -1] and t["right"].tolist() == [2, -1, -1]
    assert t["parent"].tolist() == [-1, 0 + lb, 0]
    assert t["feature"].tolist() == [1, 0, 0] and t["default_left"].tolist() == [0, 0, 0]
    assert t["value"].tolist() == [2.0, 2.0, 3.0]
    assert t["loss_chg"].tolist() == [1.0, 0.0, 0.0]
    assert t["sum_hess"].tolist() == [4.0, 2.0, 2.0], "over the bag"
    assert t["base_weight"].tolist() == [2.5, 2.0, 3.0]
    assert out["pred"].tolist() == [2, 3, 2, 3, 2, 3, 2, 3], "every row, in or out of the bag"
    assert out["train_sums"] == [72 << 72, 20 << 72] and out["train_W"] == 8 * Q
    assert out["train_rmse"] == [3.0, math.sqrt(20.0 / 8.0)]
    assert out["nodes_added"] == 3 and (out["rounds_run"], out["best_round"]) == (1, 1)
    # all features: f0 wins the root with 9
    full = P.boost_sampled(z, x, NAN, y, None, cuts, 2, **dict(kw, colsample_bytree=1.0))
    assert full["trees"][0]["feature"][0] == 0 and full["trees"][0]["loss_chg"][0] == 9.0
    # the library's host functions on the same draw
    assert synth.boost_bag(0, 0, 8, 0.5)[0].tolist() == out["bags"][0].tolist()
    assert synth.boost_features(0, 0, 2, 0.5).tolist() == [1]
    # (1, 1): the weighted restatement, whatever the seed
    a = P.boost_sampled(z, x, NAN, y, None, cuts, 2, **dict(kw, subsample=1.0, colsample_bytree=1.0, seed=99, rounds=2))
    w = W.boost_weighted(z, x, NAN, y, None, cuts, 2, rounds=2, max_depth=2, eta=1.0, lam=0.0, min_child_weight=0.0)
    assert a["train_sums"] == w["train_sums"]
    for ta, tw in zip(a["trees"], w["trees"]):
        assert all(np.array_equal(ta[k], tw[k]) for k in ta)
    # a forest that already holds a tree draws tree 1's bag: rows 0, 1, 2, 4, 5, 6, 7
    assert P.bag(0, 1, 8, 0.5).tolist() == [True, True, True, False, True, True, True, True]
    b = P.boost_sampled(z, x, NAN, y, None, cuts, 2, **dict(kw, tree0=1))
    assert b["bags"][0].tolist() == P.bag(0, 1, 8, 0.5).tolist() and b["trees"][0]["sum_hess"][0] == 7.0
    # a NaN label on an out-of-bag row is still a label refused; an empty bag says so
    yb = y.copy()
    yb[1] = np.nan
    with pytest.raises(ValueError, match="^label"):
        P.boost_sampled(z, x, NAN, yb, None, cuts, 2, **kw)
    wz = np.ones(8, np.float32)
    wz[[0, 3, 4, 5]] = 0.0
    with pytest.raises(ValueError, match="^bag"):
        P.boost_sampled(z, x, NAN, y, wz, cuts, 2, **kw)
    assert not P.bag(0, 3, 1, 0.5)[0], "one row, tree 3 of seed 0: nothing is drawn"
    with pytest.raises(ValueError, match="^bag"):
        P.boost_sampled(z[:1], x[:1], NAN, y[:1], None, cuts, 2, **dict(kw, tree0=3))
