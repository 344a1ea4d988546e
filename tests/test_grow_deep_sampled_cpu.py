"""Row and column subsampling for trees deeper than eight levels (OHXBoosterBoostTreesDeepSampled), what can be checked
without a GPU: the two entry points are declared, bound, exported and placed behind the Deep block with the Sampled call's
argument lists; the header states the semantics and its two consequences; every refusal that needs no device, in the
Sampled call's order and with max_depth refused as 1..18, outputs and saved bytes unchanged; the plan over n_sel columns
against the sampled, the weighted and the deep plans and the header's formulas; the restatement reaches what the GPU
cases are there for; the new kernels cross-compile for gfx950 with no scratch, no flat access, no float atomic, no
compare-and-swap, no LDS in the histogram kernel and the bag's word by a scalar load; and the plan under sanitizers in a
program of its own."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_deep_sampled_support as DS
from tests import grow_deep_support as D
from tests import helpers
from tests.test_grow_cpu import kernel_body, saved
from tests.test_grow_sampled_cpu import call
from tests.test_grow_weighted_cpu import call as call_weighted

HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["OHXBoosterBoostTreesDeepSampled", "OHXBoosterBoostTreesDeepSampledDevice"]
KERNELS = ["grow_deep_hist_sampled_kernel", "grow_deep_split_sampled_kernelILi0E", "grow_deep_split_sampled_kernelILi1E"]
OLD_KERNELS = ["grow_deep_widen_kernel", "grow_deep_hist_kernel", "grow_deep_split_kernelILi0E", "grow_deep_split_kernelILi1E",
               "grow_deep_partition_kernel", "grow_deep_leaf_kernel", "grow_deep_stage_kernel", "grow_deep_walk_sse_kernel"]
NAN = float("nan")


def _booster():
    js, _ = S.make_booster(11, 3)
    F = int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])
    return capi.Booster(model_buffer=js), F


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
        # directly behind the Deep block, before the cuts
        assert header.index("int OHXBoosterBoostTreesDeepDevice(") < header.index("int " + name + "(") < header.index("int OHXQuantileCuts(")
        assert f90.index('name="OHXBoosterBoostTreesDeepDevice"') < f90.index(f'name="{name}"') < f90.index('name="OHXQuantileCuts"')
        # the Sampled call's arguments, one for one
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S).group(1)
        twin = re.search(r"\bint " + name.replace("DeepSampled", "Sampled") + r"\((.*?)\);", header, re.S).group(1)
        assert re.sub(r"\s+", " ", decl) == re.sub(r"\s+", " ", twin), name
    between = header[header.index("int OHXBoosterBoostTreesDeepDevice("):header.index("int OHXBoosterBoostTreesDeepSampled(")]
    assert len(re.findall(r"^int \w+\(", between, re.M)) == 1, "nothing is declared between the Deep block and the new one"
    for method in ("boost_trees_deep_sampled", "boost_trees_deep_sampled_device"):
        assert hasattr(capi.Booster, method)
    assert hasattr(synth, "grow_plan_deep_sampled")
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.SYNTH_SO], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r" T ohx_grow_plan_deep_sampled$", nm, re.M)
    capi.load_library()
    plib = capi.Booster().lib
    assert plib.OHXBoosterBoostTreesDeepSampled.argtypes == plib.OHXBoosterBoostTreesSampled.argtypes
    assert plib.OHXBoosterBoostTreesDeepSampledDevice.argtypes == plib.OHXBoosterBoostTreesSampledDevice.argtypes


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    header = re.sub(r"\s*\n \*\s*", " ", header)          # comment lines joined
    block = header[header.index("Row and column subsampling for trees deeper than eight levels"):
                   header.index("int OHXBoosterBoostTreesDeepSampled(")]
    for phrase in ("OHXBoosterBoostTreesSampled with max_depth in 1..18", "argument for argument", "word for word",
                   "the mix function, the tree keys with T0, the bag, n_sel and the selection by (c_f, f)",
                   "every out-of-bag row has weight 0", "every unselected feature has an empty cut list",
                   "pred += leaf(row) for every row", "train_rmse, eval_rmse, W, the stop rule",
                   "refused with \"label\"", "refused with \"bag\"", "max_depth is in 1..18",
                   "min(2^(max_depth + 1) - 1, 2 * nrow - 1) nodes", "min(2^(max_depth + 1), 2 * nrow) records a round",
                   "one wait per level from level 7 on for the 16-byte level word", "enqueues no empty level",
                   "a row outside the bag makes no add", "n_sel * 256 * 16 bytes", "Integer adds only",
                   "only through r in the draw", "Launch shape, batch size, form, stream and OHXDMatrixSetGrid change nothing",
                   # the two consequences
                   "With max_depth <= 8 the forest, XGBoosterSaveModel's bytes in all three formats and both RMSE arrays equal those of OHXBoosterBoostTreesSampled",
                   "the call takes that path as it is",
                   "With subsample = colsample_bytree = 1.0f and any seed they equal those of OHXBoosterBoostTreesDeep, at any max_depth",
                   "after min_child_weight and before the cuts", "\"max_depth must be in 1..18\"", "refused with its bytes",
                   "Not capturable"):
        assert phrase in block, phrase
    # the Deep call's comment keeps its sentence, and now points here
    assert "there is no Deep form of the Sampled call. (OHXBoosterBoostTreesDeepSampled, below, has since become that form" in header


# ---- refusals that need no device ----

@pytest.mark.parametrize("name", SYMBOLS)
def test_bad_arguments_are_refused_in_the_sampled_calls_order(name):
    rc, msg = call(capi.Booster(), name)
    assert rc == -1 and "holds no model" in msg, msg
    b, F = _booster()
    before = saved(b)
    rc, msg = call(b, name, nfeat=F, labels=False)
    assert rc == -1 and name in msg and "labels is NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, cut_ptr=False)
    assert rc == -1 and "the cuts are NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, rounds=0)
    assert rc == -1 and "rounds must be >= 1" in msg, msg
    for dep in (0, 19, -3, 1 << 20):
        rc, msg = call(b, name, nfeat=F, max_depth=dep)
        assert rc == -1 and name in msg and "max_depth must be in 1..18" in msg, msg
    rc, msg = call(b, name, nfeat=F, eta=NAN, max_depth=18)
    assert rc == -1 and "eta must be finite" in msg, msg
    rc, msg = call(b, name, nfeat=F, lam=-1.0, max_depth=18)
    assert rc == -1 and "lambda must be finite and >= 0" in msg, msg
    rc, msg = call(b, name, nfeat=F, gamma=float("inf"), max_depth=9)
    assert rc == -1 and "gamma must be finite and >= 0" in msg, msg
    for bad in (NAN, float("inf"), -1.0, -1e-30):
        rc, msg = call(b, name, nfeat=F, min_child_weight=bad, max_depth=12)
        assert rc == -1 and name in msg and "min_child_weight must be finite and >= 0" in msg, msg
    tiny = float(np.float32(2.0 ** -26))             # finite and > 0, but k_s == 0
    for bad in (NAN, float("inf"), float("-inf"), 0.0, -0.5, float(np.nextafter(np.float32(1), np.float32(2))), 2.0, tiny):
        rc, msg = call(b, name, nfeat=F, subsample=bad, max_depth=18)
        assert rc == -1 and name in msg and "subsample must be finite, > 0 and <= 1" in msg, (bad, msg)
    for bad in (NAN, float("inf"), float("-inf"), 0.0, -0.5, float(np.nextafter(np.float32(1), np.float32(2))), 2.0):
        rc, msg = call(b, name, nfeat=F, colsample=bad, max_depth=18)
        assert rc == -1 and name in msg and "colsample_bytree must be finite, > 0 and <= 1" in msg, (bad, msg)
    rc, msg = call(b, name, nfeat=F, patience=-1, max_depth=12)
    assert rc == -1 and "patience must be >= 0" in msg, msg
    rc, msg = call(b, name, nfeat=F, patience=2, max_depth=12)
    assert rc == -1 and "needs a held-out matrix" in msg, msg
    # the order: rounds, max_depth, eta .. min_child_weight, subsample, colsample_bytree, the cuts, patience
    rc, msg = call(b, name, nfeat=F, rounds=0, max_depth=19)
    assert rc == -1 and "rounds must be >= 1" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=19, eta=NAN)
    assert rc == -1 and "max_depth must be in 1..18" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=19, subsample=0.0)
    assert rc == -1 and "max_depth must be in 1..18" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=18, min_child_weight=-1.0, subsample=0.0)
    assert rc == -1 and "min_child_weight" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=18, subsample=0.0, colsample=0.0)
    assert rc == -1 and "subsample must be" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=18, colsample=0.0, descending_cuts=True)
    assert rc == -1 and "colsample_bytree" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=18, subsample=0.0, patience=-1)
    assert rc == -1 and "subsample" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=18, descending_cuts=True, patience=-1)
    assert rc == -1 and "patience" not in msg and "subsample" not in msg, msg
    # every argument sound, at both ends of the depths and on either side of 8, sampled or not: the NULL matrix is left
    for dep in (1, 8, 9, 18):
        for kw in ({}, {"subsample": 2.0 ** -24, "colsample": 2.0 ** -20, "seed": (1 << 64) - 1}, {"subsample": 0.5, "colsample": 0.5},
                   {"subsample": 0.5}, {"colsample": 0.5}):
            rc, msg = call(b, name, nfeat=F, max_depth=dep, min_child_weight=0.0, **kw)
            assert rc == -1 and "DMatrix handle is invalid" in msg, (dep, kw, msg)
    assert saved(b) == before, "a refusal changed the forest"


def test_the_sampled_call_still_refuses_depth_9_and_the_deep_call_is_sound():
    b, F = _booster()
    for name in ("OHXBoosterBoostTreesSampled", "OHXBoosterBoostTreesSampledDevice"):
        rc, msg = call(b, name, nfeat=F, max_depth=9)
        assert rc == -1 and name in msg and "max_depth must be in 1..8" in msg, msg
        rc, msg = call(b, name, nfeat=F, max_depth=8, subsample=0.5)
        assert rc == -1 and "DMatrix handle is invalid" in msg, msg
    for name in ("OHXBoosterBoostTreesDeep", "OHXBoosterBoostTreesDeepDevice"):
        rc, msg = call_weighted(b, name, nfeat=F, max_depth=19)
        assert rc == -1 and name in msg and "max_depth must be in 1..18" in msg, msg
        for dep in (1, 8, 9, 18):
            rc, msg = call_weighted(b, name, nfeat=F, max_depth=dep, weights=True, min_child_weight=0.0)
            assert rc == -1 and "DMatrix handle is invalid" in msg, (dep, msg)


# ---- the plan ----

def _colsample_for(n_sel, F):
    """A colsample_bytree whose n_sel is the one asked for: floor(c * F) == n_sel."""
    c = float(np.float32(min(1.0, (n_sel + 0.5) / F)))
    assert max(1, int(np.floor(np.float64(np.float32(c)) * F))) == n_sel
    return c


@pytest.mark.parametrize("nrow", [1, 63, 64, 65, 4097, 1 << 20, 55987200, 1 << 31])
@pytest.mark.parametrize("nfeat", [1, 3, 27, 128])
def test_the_plan(nrow, nfeat):
    cus, batch = 256, synth.grow_deep_batch()
    ncuts = nfeat * 254
    for n_sel in sorted(set(range(1, min(nfeat, 8) + 1)) | {nfeat // 2 or 1, nfeat - 1 or 1, nfeat}):
        for depth in range(1, 19):
            p = synth.grow_plan_deep_sampled(nrow, nfeat, n_sel, ncuts, depth, cus)
            top = min(depth, 8)
            # levels 0 - 7 are the sampled plan's for n_sel (the weighted plan over n_sel columns, every feature's bins)
            s = synth.grow_plan_sampled(nrow, nfeat, _colsample_for(n_sel, nfeat), ncuts, top, cus)
            w = synth.grow_plan_weighted(nrow, n_sel, ncuts, top, cus)
            assert s["n_sel"] == n_sel == p["n_sel"]
            assert len(p["levels"]) == top and p["levels"] == s["levels"] == w["levels"]
            for k in ("row_blocks", "block_rows", "bin_lds_bytes", "bins_bytes", "hist_bytes", "hist_block_rows", "max_pairs", "pair_bytes"):
                assert p[k] == s[k], k
            assert p["bins_bytes"] == nfeat * nrow and p["hist_bytes"] == 2 ** (top - 1) * n_sel * 256 * 16
            # the deep levels: compact scratch and candidates, the Deep call's stride and batch
            open_max = min(2 ** (depth - 1), nrow)
            assert p["scratch_bytes"] == (min(batch, open_max) * n_sel * 256 * 16 if depth > 8 else 0)
            assert p["best_bytes"] == max(open_max, 2 ** (top - 1)) * n_sel * 32
            assert depth <= 8 or p["best_bytes"] == max(open_max, 128) * n_sel * 32
            assert p["node_stride"] == min(2 ** (depth + 1), 2 * nrow) and p["batch"] == batch == 1024
            assert p["deep_block_rows"] == 256 and 1 <= p["deep_hist_blocks"] <= cus * 8 and (p["deep_hist_blocks"] - 1) * 256 < nrow
            if n_sel == nfeat:
                q = synth.grow_plan_deep(nrow, nfeat, ncuts, depth, cus)
                assert {k: v for k, v in p.items() if k != "n_sel"} == q
    # what the flagship rows pay at half the features: 13 of 27 columns
    assert synth.grow_plan_deep_sampled(55987200, 27, 13, 6639, 18, 256)["scratch_bytes"] == 1024 * 13 * 256 * 16


def test_the_plan_refuses_what_it_cannot_plan():
    for depth in (0, 19, -1):
        with pytest.raises(Exception, match="1..18"):
            synth.grow_plan_deep_sampled(4097, 3, 2, 0, depth, 256)
    for F, n_sel in ((3, 0), (3, 4), (0, 0), (129, 5)):
        with pytest.raises(Exception, match="features"):
            synth.grow_plan_deep_sampled(4097, F, n_sel, 0, 12, 256)
    with pytest.raises(Exception, match="no rows"):
        synth.grow_plan_deep_sampled(0, 3, 2, 0, 12, 256)


# ---- the restatement reaches what the GPU cases are there for ----

def test_the_restatement_reaches_several_batches_over_a_bag_and_a_list():
    """40 000 rows of 5 features, depth 14, half the rows and 3 of the 5 features."""
    x, y, w, cuts, ev, want = DS.restated(40000, 40014, 14, 64, 0.0, 0.0, 0.5, 0.7, 5, rounds=1, nfeat=5)
    batch = synth.grow_deep_batch()
    t, bag, feats = want["trees"][0], want["bags"][0], want["features"][0]
    lv = D.levels(t)
    assert len(feats) == 3 < 5 and feats == sorted(feats)
    assert 0 < int(bag.sum()) < 40000 and abs(int(bag.sum()) - 20000) < 600, "a bag strictly inside the rows, about half"
    assert D.depth_of(t) == 14 and all(splits > 0 for _, splits in lv[:14])
    assert sum(o > batch for o, _ in lv) >= 2, "levels with more open nodes than a batch holds"
    assert max(o for o, _ in lv[8:]) > 256, "several chunks of phase 1"
    assert set(t["feature"][t["left"] >= 0].tolist()) <= set(feats)
    assert len(t["left"]) == 1 + 2 * sum(s for _, s in lv) <= 2 * int(bag.sum()) - 1, "every leaf holds a row of the bag"
    assert float(t["sum_hess"][0]) == float(bag.sum()), "the root's sum is over the bag"


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_deep.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_deep.hip")
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
def test_deep_sampled_kernels_resources_and_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    assert _figure(report, kernel, "VGPRs Spill") == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    lds = _figure(report, kernel, "LDS Size [bytes/block]")
    vgprs, occupancy = _figure(report, kernel, "VGPRs"), _figure(report, kernel, "Occupancy [waves/SIMD]")
    if "hist" in kernel:
        adds = [l for l in body.splitlines() if "global_atomic_add_x2" in l]
        # two adds a feature over the 32 columns a block takes, and they return nothing
        assert len(adds) == 2 * 32 and not any("sc0" in l for l in adds)
        assert "ds_" not in body and lds == 0, "no LDS"
        assert "global_atomic_add " not in body and "global_atomic_add_u32" not in body
        # the bag's word: a scalar load of 64 bits; no lane loads 64 bits of anything
        assert "s_load_dwordx2" in body and "global_load_dwordx2" not in body
        assert re.search(r"v_readfirstlane_b32[^\n]*\n(?:[^\n]*\n){0,12}?\s*s_load_dwordx2", body), "the word index is made wave-uniform, then loaded"
        # the bins: one byte load a column, and the features read once, a byte each
        assert len(re.findall(r"global_load_ubyte", body)) == 2 * 32
        assert vgprs <= 64 and occupancy == 8, (vgprs, occupancy)
    else:
        assert "atomic_add" not in body and "ds_add" not in body
        assert lds == (4 * 4 if "ILi1E" in kernel else 0)
        assert vgprs <= 128 and occupancy >= 4, (vgprs, occupancy)
    if "ILi0E" in kernel:
        assert "v_div_scale_f64" in body, "the gain divides in double"


def test_the_new_kernels_hide_no_old_name_and_share_the_chunk_loop(isa):
    text, _ = isa
    symbols = re.findall(r"^(_Z\w+):\s*; @\1$", text, re.M)
    for old in OLD_KERNELS:
        hits = [s for s in symbols if old in s]
        assert len(hits) == 1, (old, hits)
    for new in KERNELS:
        assert len([s for s in symbols if new in s]) == 1, new
    assert len(symbols) == len(OLD_KERNELS) + len(KERNELS)
    # the chunk loop of split phase 1 is written once
    src = open(os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_deep.hip")).read()
    assert len(re.findall(r"for \(uint32_t c0 = 0;", src)) == 1


# ---- the plan under sanitizers ----

def test_the_plan_under_sanitizers(tmp_path):
    """tools/grow_deep_sampled_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only): the
    plan over 1 to 2^31 rows, 1 to 128 features, every n_sel and every depth."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_deep_sampled_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_deep_sampled_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
