"""Trees deeper than eight levels (OHXBoosterBoostTreesDeep), what can be checked without a GPU: the two entry points are
declared, bound, exported and placed; the header states the semantics; every refusal that needs no device, in the
Weighted call's order and with max_depth refused as 1..18, outputs and saved bytes unchanged; the plan (levels 0 - 7
equal the weighted plan, the scratch is bounded by the batch, the node stride follows its formula); the chunked child-id
assignment of split phase 1 through its host build against a plain loop; the new kernels cross-compile for gfx950 with
no scratch, no flat access, no float atomic and no compare-and-swap, and the histogram kernel adds with 64-bit integer
global adds and no LDS; and the level view of tests/grow_deep_support.py on a tree worked by hand."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_deep_support as D
from tests import helpers
from tests.test_grow_cpu import kernel_body, saved
from tests.test_grow_weighted_cpu import call

HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["OHXBoosterBoostTreesDeep", "OHXBoosterBoostTreesDeepDevice"]
KERNELS = ["grow_deep_widen_kernel", "grow_deep_hist_kernel", "grow_deep_split_kernelILi0E", "grow_deep_split_kernelILi1E",
           "grow_deep_partition_kernel", "grow_deep_leaf_kernel", "grow_deep_stage_kernel", "grow_deep_walk_sse_kernel"]
BLOCK = 256          # lanes of the block that hands out the child ids (csrc/grow.hpp kGrowBlock)


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
        # behind the Sampled block
        assert header.index("int OHXBoosterBoostTreesSampledDevice(") < header.index("int " + name + "(") < header.index("int OHXQuantileCuts(")
        assert f90.index('name="OHXBoosterBoostTreesSampledDevice"') < f90.index(f'name="{name}"')
    for method in ("boost_trees_deep", "boost_trees_deep_device"):
        assert hasattr(capi.Booster, method)
    for f in ("grow_plan_deep", "grow_deep_batch", "grow_deep_children"):
        assert hasattr(synth, f)
    # the argument lists are the Weighted call's
    capi.load_library()
    plib = capi.Booster().lib
    assert plib.OHXBoosterBoostTreesDeep.argtypes == plib.OHXBoosterBoostTreesWeighted.argtypes
    assert plib.OHXBoosterBoostTreesDeepDevice.argtypes == plib.OHXBoosterBoostTreesWeightedDevice.argtypes


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    header = re.sub(r"\s*\n \*\s*", " ", header)          # comment lines joined
    for phrase in ("OHXBoosterBoostTreesWeighted with max_depth in 1..18", "word for word", "max_depth is in 1..18",
                   "nothing deeper has run", "HL > 0 and HR > 0, so every leaf holds a row",
                   "min(2^(max_depth + 1) - 1, 2 * nrow - 1) nodes", "min(2^(max_depth + 1), 2 * nrow) records a round",
                   "the scratch does not grow with the depth", "cannot change a bit",
                   "With max_depth <= 8 the forest, XGBoosterSaveModel's bytes in all three formats and both RMSE arrays equal those of OHXBoosterBoostTreesWeighted",
                   "min_child_weight = (float)min_child_rows they equal those of OHXBoosterBoostTreesEval",
                   "once per level from level 7 on for the 16-byte level word", "enqueues no empty level",
                   "Levels below 7 read nothing back", "there is no Deep form of the Sampled call",
                   "\"max_depth must be in 1..18\"", "refused with its bytes"):
        assert phrase in header, phrase


# ---- refusals that need no device ----

@pytest.mark.parametrize("name", SYMBOLS)
def test_no_model_is_refused(name):
    rc, msg = call(capi.Booster(), name)
    assert rc == -1 and "holds no model" in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
def test_bad_arguments_are_refused_in_the_weighted_calls_order(name):
    js, _ = S.make_booster(11, 3)
    F = int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])
    b = capi.Booster(model_buffer=js)
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
    rc, msg = call(b, name, nfeat=F, eta=float("nan"), max_depth=18)
    assert rc == -1 and "eta must be finite" in msg, msg
    rc, msg = call(b, name, nfeat=F, lam=-1.0, max_depth=18)
    assert rc == -1 and "lambda must be finite and >= 0" in msg, msg
    rc, msg = call(b, name, nfeat=F, gamma=float("inf"), max_depth=9)
    assert rc == -1 and "gamma must be finite and >= 0" in msg, msg
    for bad in (float("nan"), float("inf"), -1.0, -1e-30):
        rc, msg = call(b, name, nfeat=F, min_child_weight=bad, max_depth=12)
        assert rc == -1 and name in msg and "min_child_weight must be finite and >= 0" in msg, msg
    rc, msg = call(b, name, nfeat=F, patience=-1, max_depth=12)
    assert rc == -1 and "patience must be >= 0" in msg, msg
    for kw in ({"run": False}, {"best": False}):
        rc, msg = call(b, name, nfeat=F, max_depth=12, **kw)
        assert rc == -1 and "rounds_run or best_round is NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, patience=2, max_depth=12)
    assert rc == -1 and "needs a held-out matrix" in msg, msg
    rc, msg = call(b, name, nfeat=F, eval_labels=True, eval_nlabel=4, max_depth=12)
    assert rc == -1 and "eval labels are given without a held-out matrix" in msg, msg
    rc, msg = call(b, name, nfeat=F, eval_weights=True, max_depth=12)
    assert rc == -1 and "eval weights are given without a held-out matrix" in msg, msg
    rc, msg = call(b, name, nfeat=F, eval_dmat=C.c_void_p(0x1000), eval_nlabel=4, eval_weights=True, max_depth=18)
    assert rc == -1 and "eval labels is NULL" in msg, msg
    # an earlier refusal wins over a later one
    rc, msg = call(b, name, nfeat=F, rounds=0, max_depth=19)
    assert rc == -1 and "rounds must be >= 1" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=19, eta=float("nan"))
    assert rc == -1 and "max_depth must be in 1..18" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=19, min_child_weight=-1.0)
    assert rc == -1 and "max_depth must be in 1..18" in msg, msg
    # every argument sound, at both ends of the depths and on either side of 8: the NULL matrix is what is left
    for dep in (1, 8, 9, 18):
        rc, msg = call(b, name, nfeat=F, max_depth=dep, weights=True, min_child_weight=0.0)
        assert rc == -1 and "DMatrix handle is invalid" in msg, (dep, msg)
    assert saved(b) == before, "a refusal changed the forest"


def test_the_weighted_call_still_refuses_depth_9():
    js, _ = S.make_booster(11, 3)
    F = int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])
    b = capi.Booster(model_buffer=js)
    for name in ("OHXBoosterBoostTreesWeighted", "OHXBoosterBoostTreesWeightedDevice"):
        rc, msg = call(b, name, nfeat=F, max_depth=9)
        assert rc == -1 and "max_depth must be in 1..8" in msg, msg


# ---- the plan ----

@pytest.mark.parametrize("nrow", [1, 63, 64, 65, 4097, 1 << 20, 55987200, 1 << 31])
@pytest.mark.parametrize("nfeat", [1, 3, 27, 41, 128])
def test_the_plan(nrow, nfeat):
    cus, batch = 256, synth.grow_deep_batch()
    assert batch == 1024
    for depth in range(1, 19):
        p = synth.grow_plan_deep(nrow, nfeat, nfeat * 254, depth, cus)
        w = synth.grow_plan_weighted(nrow, nfeat, nfeat * 254, min(depth, 8), cus)
        # levels 0 - 7 are the weighted plan's
        assert len(p["levels"]) == min(depth, 8) and p["levels"] == w["levels"]
        for k in ("row_blocks", "block_rows", "bin_lds_bytes", "bins_bytes", "hist_bytes", "hist_block_rows", "max_pairs", "pair_bytes"):
            assert p[k] == w[k], k
        # the node stride, and a tree's nodes within it
        assert p["node_stride"] == min(2 ** (depth + 1), 2 * nrow)
        assert min(2 ** (depth + 1) - 1, 2 * nrow - 1) < p["node_stride"]
        # the open nodes of a level: at most half the next level's slots, and a row each
        open_max = min(2 ** (depth - 1), nrow)
        assert p["best_bytes"] == max(open_max, 2 ** (min(depth, 8) - 1)) * nfeat * 32
        assert p["batch"] == batch
        if depth <= 8:
            assert p["scratch_bytes"] == 0
        else:
            # bounded by the batch whatever the depth: 16 bytes a bin, 256 bins a (slot, feature)
            assert p["scratch_bytes"] == min(batch, open_max) * nfeat * 256 * 16 <= batch * nfeat * 256 * 16
            if nrow >= 1 << 20 and depth >= 12:
                assert p["scratch_bytes"] == batch * nfeat * 256 * 16
        # the global histogram kernel: a row per lane, no more blocks than rows need
        assert p["deep_block_rows"] == 256
        assert 1 <= p["deep_hist_blocks"] <= cus * 8 and (p["deep_hist_blocks"] - 1) * 256 < nrow
    assert synth.grow_plan_deep(55987200, 27, 6639, 18, 256)["scratch_bytes"] == 113246208, "113 MB at 27 features"


def test_the_plan_refuses_other_depths():
    for depth in (0, 19, -1):
        with pytest.raises(Exception, match="1..18"):
            synth.grow_plan_deep(4097, 3, 0, depth, 256)


# ---- the chunked child ids of split phase 1 ----

def _plain_children(flags, next_id):
    left, below = np.zeros(len(flags), np.uint32), 0
    for s, f in enumerate(flags):
        if f:
            left[s] = next_id + 2 * below
            below += 1
    return left, below


def test_chunked_child_ids_equal_a_plain_loop():
    batch = synth.grow_deep_batch()
    rng = np.random.default_rng(5)
    counts = [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1, batch - 1, batch, batch + 1, 3 * batch + 77]
    for count in counts:
        patterns = [np.zeros(count, np.uint8), np.ones(count, np.uint8), (np.arange(count) % 2).astype(np.uint8),
                    (rng.random(count) < 0.5).astype(np.uint8), (rng.random(count) < 0.03).astype(np.uint8)]
        if count > BLOCK:
            edge = np.zeros(count, np.uint8)          # splits on both sides of every chunk border only
            edge[BLOCK - 1::BLOCK] = 1
            edge[BLOCK::BLOCK] = 1
            patterns.append(edge)
        for flags in patterns:
            for next_id in (1, 511, 123457):
                want, nwant = _plain_children(flags, next_id)
                for width in (BLOCK, 64, 1, batch + 5):
                    got, n = synth.grow_deep_children(flags, width, next_id)
                    assert n == nwant == int(flags.sum()), (count, width)
                    assert np.array_equal(got, want), (count, width, next_id)
                # ids ascend in node order, two apart, from next_id: the children of a level are contiguous
                ids = want[flags != 0]
                assert np.array_equal(ids, next_id + 2 * np.arange(len(ids)))


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
def test_deep_kernels_resources_and_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    lds = _figure(report, kernel, "LDS Size [bytes/block]")
    if "hist" in kernel:
        assert "global_atomic_add_x2" in body, "64-bit integer global adds"
        adds = [l for l in body.splitlines() if "global_atomic_add_x2" in l]
        assert len(adds) == 2 and not any("sc0" in l for l in adds), "two adds a feature, and they return nothing"
        assert "ds_" not in body and lds == 0, "no LDS"
        assert "global_atomic_add " not in body and "global_atomic_add_u32" not in body
    elif "walk_sse" in kernel:
        assert "global_atomic_add_x2" in body and "ds_add" not in body
        assert lds == 4 * 4 * 8, "the reduction's partial sums alone: no tree is staged"
    else:
        assert "atomic_add" not in body and "ds_add" not in body
        assert lds == (4 * 4 if "ILi1E" in kernel else 0)
    if "ILi0E" in kernel:
        assert "v_div_scale_f64" in body, "the gain divides in double"


# ---- the level view of the support ----

def test_the_level_view_on_a_tree_by_hand():
    # 0 -> (1, 2); 1 -> (3, 4); 2 a leaf; 3 a leaf; 4 -> (5, 6)
    t = {"left": np.array([1, 3, -1, -1, 5, -1, -1], np.int32), "right": np.array([2, 4, -1, -1, 6, -1, -1], np.int32)}
    assert D.levels(t) == [(1, 1), (2, 1), (2, 1), (2, 0)] and D.depth_of(t) == 3
    assert D.levels({"left": np.array([-1], np.int32), "right": np.array([-1], np.int32)}) == [(1, 0)]


def test_the_restatement_goes_past_depth_8():
    x, y, w, cuts, ev, want = D.restated(4097, 4097, 12, 255, 1.0, 0.0)
    t = want["trees"][0]
    lv = D.levels(t)
    assert D.depth_of(t) == 12 and all(s > 0 for _, s in lv[:12]) and lv[12][1] == 0
    assert len(t["left"]) == 1 + 2 * sum(s for _, s in lv) <= min(2 ** 13 - 1, 2 * 4097 - 1)
    assert cuts[0][-1] == len(cuts[1]) and x.shape == (4097, 3) and w is None and ev is None
