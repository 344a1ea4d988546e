""""ohx_interaction_constraints" without a GPU (csrc/grow.hpp grow_interact_allowed; csrc/grow.cpp grow_interact_parse; the
parameter and the refusals in csrc/capi.cpp): the grammar, a node's allowed set against a set-based version, the refusals
that need no device, the auditor on a hand-made tree, the condition that gives the GPU tests their teeth, the cross-compiled
kernels' resources, and the host code under AddressSanitizer and UBSan."""
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
from tests import grow_interact_support as I
from tests import helpers
from tests.test_grow_colsample_cpu import _figure
from tests.test_grow_cpu import kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
NAME = "ohx_interaction_constraints"
POLICIES = ("GrowFixedHess", "GrowRegHess", "GrowMonoArgs")
KERNELS = [f"grow_split_interact_kernelINS_{len(p)}{p}E{v}" for p in POLICIES for v in ("Li0ELi0E", "Li1ELi0E", "Li1ELi1E", "Li1ELi2E")] + \
          [f"grow_deep_split_interact_kernelINS_{len(p)}{p}E{v}" for p in POLICIES for v in ("Li0E", "Li1E")]
# the VGPRs of docs/35_interaction_constraints.md 35.2: phase 0 and phase 1 of levels 0 - 7, then of the deep levels
VGPRS = {"GrowFixedHess": (70, 58, 70, 70), "GrowRegHess": (74, 60, 72, 80), "GrowMonoArgs": (83, 64, 82, 96)}

SIXTY_FOUR = "[" + ",".join("[%d,%d]" % (g, g + 64) for g in range(64)) + "]"
GOOD = ("[]", " [ ] ", str([[0, 2], [1, 3, 4]]), "[[0]]", "[[127]]", "[[63,64,127]]", "\t[\t[ 007 ]\t]", "[[1],[1],[1,2]]", SIXTY_FOUR)
BAD = ("", " ", "[[]]", "[0, 1]", "[[0, 0]]", "[[1.0]]", "[[-1]]", "[[+1]]", "[[0],]", "[[0,]]", "[[0]],", "[[0]] x", "[[0] [1]]", "[[128]]",
       "[[4294967296]]", "[[0]", "((0))", "[[[0]]]", SIXTY_FOUR[:-1] + ",[0]]")


def c_call(b, name, nfeat, dmat=None, labels=None, nlabel=4, weights=None):
    """One boost entry point, any of the six in either form, through the C interface with every output poisoned -> (rc,
    message); asserts that no output was written.  Without a matrix the call ends at the matrix's refusal at the latest.
    labels / weights: addresses the form can read (the host's by default)."""
    y = np.zeros(4, np.float32)
    ptr, vals = np.arange(nfeat + 1, dtype=np.uint64), np.arange(nfeat, dtype=np.float32)
    train, evals = np.full(3, -7.0), np.full(3, -7.0)
    run, best, added = C.c_int32(-7), C.c_int32(-7), C.c_uint64(77)
    labels = labels if labels is not None else y.ctypes.data
    base = name[:-6] if name.endswith("Device") else name
    outs = [train.ctypes.data, evals.ctypes.data, C.byref(run), C.byref(best), C.byref(added)]
    if base == "OHXBoosterBoostTrees":
        args = [b.handle, dmat, labels, nlabel, ptr.ctypes.data, vals.ctypes.data, 2, 3, 0.5, 1.0, 0.0, 1, C.byref(added)]
    elif base == "OHXBoosterBoostTreesEval":
        args = [b.handle, dmat, labels, nlabel, None, None, 0, ptr.ctypes.data, vals.ctypes.data, 2, 3, 0.5, 1.0, 0.0, 1, 0] + outs
    else:
        args = [b.handle, dmat, labels, weights, nlabel, None, None, None, 0, ptr.ctypes.data, vals.ctypes.data, 2, 3, 0.5, 1.0, 0.0, 0.0]
        if base.endswith("Sampled"):
            args += [0.75, 1.0, 5]
        args += [0] + outs
    if name.endswith("Device"):
        args.append(None)
    rc = getattr(b.lib, name)(*args)
    assert np.all(train == -7.0) and np.all(evals == -7.0) and run.value == -7 and best.value == -7 and added.value == 77, name
    return rc, b.lib.XGBGetLastError().decode()


# ---- the grammar ----

def test_the_grammar():
    for v in GOOD:
        groups, _ = synth.interact_parse(v, 128)
        assert groups == I.parse(v), v
    for v in BAD:
        with pytest.raises(ValueError):
            I.parse(v)
        with pytest.raises(RuntimeError):
            synth.interact_parse(v, 128)
    assert len(I.parse(SIXTY_FOUR)) == 64 and I.parse(I.text(I.OVERLAP)) == [list(g) for g in I.OVERLAP]
    # active: no group, or a group of every feature, is the default
    for v, F, want in (("[]", 6, False), ("[[0,1,2],[3,4,5]]", 6, True), ("[[0,1],[5,4,3,2,1,0]]", 6, False), ("[[0,1],[5,4,3,2,1,0]]", 7, True),
                       ("[[0]]", 1, False), ("[[0]]", 2, True)):
        assert synth.interact_parse(v, F)[1] is want is I.active(I.parse(v), F), (v, F)


def test_the_parameter_on_the_handle():
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    nfeat = int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])
    before = saved(b)
    for v in GOOD:
        b.set_param(NAME, v)
    b.set_param(NAME, "[[0],[1]]")
    for v in BAD:
        with pytest.raises(capi.OhxError, match=NAME):
            b.set_param(NAME, v)
        rc, msg = c_call(b, "OHXBoosterBoostTrees", nfeat)            # a refused value leaves the previous one in force
        assert rc == -1 and NAME in msg and "OHXBoosterBoostTreesWeighted" in msg, (v, msg)
    b.set_param("interaction_constraints", "anything")                 # the name without the prefix stays accepted and ignored
    assert saved(b) == before, "the parameter is written into no model"
    b.free()


# ---- a node's allowed set ----

def test_allowed_against_the_sets():
    rng = np.random.default_rng(3500)
    cases = [(I.OVERLAP, 6, p) for p in ((), (0,), (1,), (2,), (3,), (4,), (1, 2), (0, 1), (0, 2), (4, 5), (1, 2, 3))]
    cases += [(((63, 64), (64, 127), (0, 63)), 128, p) for p in ((63,), (64,), (127,), (63, 64), (64, 127), (0,), (63, 127), ())]
    many = tuple((g, g + 64) for g in range(64))
    cases += [(many, 128, p) for p in ((0,), (63,), (127,), (5, 69), (5, 70), ())]
    for _ in range(300):
        F = int(rng.integers(1, 129))
        groups = tuple(tuple(int(f) for f in rng.choice(F, int(rng.integers(1, min(F, 8) + 1)), replace=False)) for _ in range(int(rng.integers(0, 65))))
        path = tuple(int(f) for f in rng.choice(F, int(rng.integers(0, min(F, 3) + 1)), replace=False))
        cases.append((groups, F, path))
    for groups, F, path in cases:
        assert synth.interact_allowed(path, groups, F) == I.allowed(path, groups, F), (groups, F, path)
    assert I.allowed({4}, I.OVERLAP, 6) == {4}, "a feature in no group admits only the path's own features"
    assert I.allowed({1}, I.OVERLAP, 6) == {0, 1, 2, 3} and I.allowed({1, 2}, I.OVERLAP, 6) == {1, 2, 3}
    assert I.allowed({0, 3}, I.OVERLAP, 6) == {0, 3}


# ---- the refusals that need no device ----

COUNT_CALLS = [base + form for base in ("OHXBoosterBoostTrees", "OHXBoosterBoostTreesEval") for form in ("", "Device")]
WEIGHT_CALLS = [base + form for base in ("OHXBoosterBoostTreesWeighted", "OHXBoosterBoostTreesDeep", "OHXBoosterBoostTreesSampled",
                                         "OHXBoosterBoostTreesDeepSampled") for form in ("", "Device")]


@pytest.mark.parametrize("name", COUNT_CALLS + WEIGHT_CALLS)
def test_refusals_at_the_top(name):
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    nfeat = int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])
    assert 3 <= nfeat < 127
    before = saved(b)
    # an id that is no feature of the booster: every call, active or not
    b.set_param(NAME, "[[0,%d]]" % nfeat)
    rc, msg = c_call(b, name, nfeat)
    assert rc == -1 and NAME in msg and name in msg and "nothing was enqueued" in msg, msg
    # active groups: the calls that keep row counts name the weighted call; the others go on to the matrix
    b.set_param(NAME, "[[0,1],[2]]")
    rc, msg = c_call(b, name, nfeat)
    if name in COUNT_CALLS:
        assert rc == -1 and NAME in msg and "OHXBoosterBoostTreesWeighted" in msg and "nothing was enqueued" in msg, msg
    else:
        assert rc == -1 and NAME not in msg and "DMatrix" in msg, msg
        if "Deep" not in name:        # (the Deep call refuses the quantile objective itself, before any handle parameter)
            b.set_param("ohx_objective", "quantile")
            rc, msg = c_call(b, name, nfeat)
            assert rc == -1 and NAME in msg and "nothing was enqueued" in msg, msg
            b.set_param("ohx_objective", "squarederror")
        if "Sampled" in name:         # the level and node fractions, where they take a feature away
            for fraction in ("ohx_colsample_bylevel", "ohx_colsample_bynode"):
                b.set_param(fraction, "0.5")
                rc, msg = c_call(b, name, nfeat)
                assert rc == -1 and NAME in msg and fraction in msg and "nothing was enqueued" in msg, msg
                b.set_param(fraction, "1")
    # inactive: the default's path, whose next refusal is the matrix's
    for v in ("[]", "[[%s]]" % ",".join(str(f) for f in range(nfeat))):
        b.set_param(NAME, v)
        rc, msg = c_call(b, name, nfeat)
        assert rc == -1 and NAME not in msg and "DMatrix" in msg, (v, msg)
    assert saved(b) == before, "a refusal changed the forest"
    b.free()


def test_the_abi_is_what_it_was():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    names = re.findall(r"^(?:int|const char\*|void)\s+((?:XG|OHX)\w+)\(", header, re.M)
    assert sorted(names) == sorted(capi.ABI_SYMBOLS) and len(names) == 78
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    for hidden in ("ohx_grow_interact", "grow_interact_splits", "grow_interact_parse", "GrowInteract"):
        assert hidden not in nm and hidden not in " ".join(capi.ABI_SYMBOLS), hidden
    assert header.index('"' + NAME + '"') < header.index("int XGBoosterSetParam(")
    for said in ("P(root) = {}", "A(root) = every feature 0 .. F - 1", "P(c) = P(p) + {f}", "C1.", "C2.", "C3.", "C4."):
        assert said in header, said


# ---- the auditor, and the condition that gives the GPU tests their teeth ----

def test_the_auditor_rejects_a_tree_that_mixes_groups():
    #        0: x0          a path x0, x3 crosses TWO_GROUPS; x0, x1 does not
    #   1: x3     2: x1
    left = np.array([1, 3, 5, -1, -1, -1, -1], np.int32)
    right = np.where(left >= 0, left + 1, -1).astype(np.int32)
    feature = np.array([0, 3, 1, 0, 0, 0, 0], np.uint32)
    assert I.tree_violations(left, right, feature, I.TWO_GROUPS, 6) == [(1, 3, [0, 1, 2])]
    assert I.tree_violations(left, right, np.array([0, 2, 1, 0, 0, 0, 0], np.uint32), I.TWO_GROUPS, 6) == []
    assert I.tree_violations(left, right, feature, (), 6) == [(1, 3, [0]), (2, 1, [0])], "no group: the path's own features alone"
    assert I.tree_violations(left, right, feature, I.SINGLETONS, 6) == [(1, 3, [0]), (2, 1, [0])]
    assert sorted(map(sorted, I.path_features(left, right, feature))) == [[0, 1], [0, 1], [0, 3], [0, 3]]


def test_free_trees_mix_the_groups_and_constrained_ones_do_not():
    for depth in (3, 8):
        *_, free = I.restated((), 4097, 351, depth)
        assert I.violations(free["trees"], I.TWO_GROUPS, I.NFEAT), "the labels' product makes a free tree mix the groups"
        for groups in (I.TWO_GROUPS, I.OVERLAP, I.SINGLETONS):
            *_, want = I.restated(groups, 4097, 351, depth)
            assert I.violations(want["trees"], groups, I.NFEAT) == [] and len(want["trees"]) == 2
            assert I.violations(free["trees"], groups, I.NFEAT), groups
            assert want["nodes_added"] > 2 * 7
            for t in want["trees"]:
                for path in I.path_features(t["left"], t["right"], t["feature"]):
                    assert len(path) <= 1 or any(path <= set(g) for g in groups), (groups, path)
                if groups == I.SINGLETONS:
                    assert len(set(t["feature"][t["left"] >= 0].tolist())) == 1, "C3"


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_interact.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_interact.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read(), r.stderr


@pytest.mark.parametrize("kernel", KERNELS)
def test_interact_kernels_resources_and_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    assert _figure(report, kernel, "VGPRs Spill") == 0 and _figure(report, kernel, "SGPRs Spill") == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body and "atomic_add" not in body and "ds_add" not in body
    atomics = set(re.findall(r"\b(?:global|ds|buffer)_atomic_\w+|\bds_(?:or|and|xor|min|max|inc|dec)\w*", body))
    assert atomics <= {"global_atomic_or"}, ("no atomic beyond the error word's or", atomics)
    policy = next(p for p in POLICIES if p in kernel)
    deep, phase = "deep" in kernel, int(re.search(r"[a-z]ELi(\d)E", kernel).group(1))
    assert _figure(report, kernel, "VGPRs") == VGPRS[policy][2 * deep + phase], "the chapter's register counts"
    assert _figure(report, kernel, "Occupancy [waves/SIMD]") >= 4


def test_the_file_holds_its_own_kernels_and_reuses_the_rest(isa):
    text, _ = isa
    symbols = re.findall(r"^(_Z\w+):\s*; @\1$", text, re.M)
    for k in KERNELS:
        assert len([s for s in symbols if k in s]) == 1, k
    assert len(symbols) == len(KERNELS) == 18
    csrc = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    src = open(os.path.join(csrc, "grow_interact.hip")).read()
    assert "grow_split_columns(" in src and "grow_split_nodes<" in src and "grow_deep_split_chunks(" in src
    for own in ("__shfl", "r.base_weight", "hipMemsetAsync", "hipStreamSynchronize", "for (uint32_t c0", "Ghist", "bins[", "hipFuncSetAttribute",
                "grow_gain", "loss_chg"):
        assert own not in src, own
    assert "-ffp-contract=off" in re.search(r"grow_interact_kernels\.o:.*\n\t.*", open(os.path.join(csrc, "Makefile")).read()).group(0)


# ---- the host functions under sanitizers ----

def test_the_parser_and_the_sets_under_sanitizers(tmp_path):
    """tools/grow_interact_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_interact_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_interact_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert re.search(r"\d+ values, \d+ sets, 0 failures", r.stdout), r.stdout
