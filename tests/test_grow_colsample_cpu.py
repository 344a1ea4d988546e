""""ohx_colsample_bylevel" and "ohx_colsample_bynode" without a GPU (csrc/grow.hpp grow_level_key, grow_node_key,
grow_node_has_feature; csrc/grow.cpp grow_pick_level_features, grow_pick_node_features; the parameters' grammar and the
refusals in csrc/capi.cpp): the host exports against the restatement (tests/grow_colsample_support.py), key ties forced
by hand, the nesting, the inclusion frequencies, a case worked by hand, the cross-compiled kernels' resources, and the
host code under AddressSanitizer and UBSan."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_colsample_support as K
from tests import grow_support as G
from tests import helpers
from tests.test_grow_cpu import kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
NAMES = ("ohx_colsample_bylevel", "ohx_colsample_bynode")
POLICIES = ("GrowFixedHess", "GrowRegHess", "GrowMonoArgs")
# <policy, phase, root> of levels 0 - 7 and <policy, phase> of the deep levels
KERNELS = [f"grow_split_colsample_kernelINS_{len(p)}{p}E{v}" for p in POLICIES for v in ("Li0ELi0E", "Li1ELi0E", "Li1ELi1E", "Li1ELi2E")] + \
          [f"grow_deep_split_colsample_kernelINS_{len(p)}{p}E{v}" for p in POLICIES for v in ("Li0E", "Li1E")]
SEEDS = (0, 1, 42, 2 ** 63 + 5)
TREES = (0, 1, 2, 3, 2 ** 32 + 1)
LEVELS = (0, 7, 8, 17)
NODES = (0, 1, 510, 511, 2 ** 19 - 1)
LISTS = (1, 2, 3, 27, 64, 65, 128)
FRACTIONS = (2.0 ** -20, 0.01, 0.3, 0.34, 0.5, 0.75, 0.99, 1.0)


# ---- the parameters, which need no device ----

GOOD = ("1", "1.0", "0.5", "1e-3", "9.5367431640625e-07", "0.34", "1e0", "+0.25", ".5")
BAD = ("", " ", "0", "0.0", "-0.5", "-1", "1.0001", "2", "nan", "inf", "-inf", "half", "0.5x", "0.5 ", "1e-60")


def test_the_grammar_of_both_parameters():
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    for name in NAMES:
        for v in GOOD:
            K.fraction(float(v), name)
            b.set_param(name, v)
        for v in BAD:
            with pytest.raises(capi.OhxError, match=name):
                b.set_param(name, v)
    for v in ("0", "nan", "-1", "7"):
        with pytest.raises(ValueError):
            K.fraction(float(v), "fraction")
    b.set_param("colsample_bylevel", "anything")       # the names without the prefix stay accepted and ignored
    b.set_param("colsample_bynode", "7")
    assert saved(b) == before, "the parameters are written into no model"
    b.free()


def c_call(b, name, nfeat):
    """One unsampled entry point through the C interface with every output poisoned and no matrix -> (rc, message); asserts
    that no output was written."""
    y = np.zeros(4, F32)
    ptr, vals = np.arange(nfeat + 1, dtype=np.uint64), np.arange(nfeat, dtype=F32)
    train, evals = np.full(3, -7.0), np.full(3, -7.0)
    run, best, added = C.c_int32(-7), C.c_int32(-7), C.c_uint64(77)
    base = name[:-6] if name.endswith("Device") else name
    if base == "OHXBoosterBoostTrees":
        args = [b.handle, None, y.ctypes.data, 4, ptr.ctypes.data, vals.ctypes.data, 2, 3, 0.5, 1.0, 0.0, 1, C.byref(added)]
    elif base == "OHXBoosterBoostTreesEval":
        args = [b.handle, None, y.ctypes.data, 4, None, None, 0, ptr.ctypes.data, vals.ctypes.data, 2, 3, 0.5, 1.0, 0.0, 1, 0,
                train.ctypes.data, evals.ctypes.data, C.byref(run), C.byref(best), C.byref(added)]
    else:
        args = [b.handle, None, y.ctypes.data, None, 4, None, None, None, 0, ptr.ctypes.data, vals.ctypes.data, 2, 3, 0.5, 1.0, 0.0, 0.0, 0,
                train.ctypes.data, evals.ctypes.data, C.byref(run), C.byref(best), C.byref(added)]
    if name.endswith("Device"):
        args.append(None)
    rc = getattr(b.lib, name)(*args)
    assert np.all(train == -7.0) and np.all(evals == -7.0) and run.value == -7 and best.value == -7 and added.value == 77, name
    return rc, b.lib.XGBGetLastError().decode()


UNSAMPLED = [base + form for base in ("OHXBoosterBoostTrees", "OHXBoosterBoostTreesEval", "OHXBoosterBoostTreesWeighted", "OHXBoosterBoostTreesDeep")
             for form in ("", "Device")]


@pytest.mark.parametrize("name", UNSAMPLED)
def test_the_calls_without_a_seed_are_refused_at_the_top(name):
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    nfeat = int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])
    before = saved(b)
    for params in ((("ohx_colsample_bylevel", "0.5"),), (("ohx_colsample_bynode", "0.99"),),
                   (("ohx_colsample_bylevel", "0.25"), ("ohx_colsample_bynode", "0.5"))):
        for k in NAMES:
            b.set_param(k, "1")
        for k, v in params:
            b.set_param(k, v)
        rc, msg = c_call(b, name, nfeat)
        assert rc == -1 and "OHXBoosterBoostTreesSampled" in msg and name in msg and "nothing was enqueued" in msg, msg
    assert saved(b) == before, "a refusal changed the forest"
    # a refused value leaves the handle's setting, and both back at 1 lift the refusal: the next one is the matrix's
    with pytest.raises(capi.OhxError, match="ohx_colsample_bynode"):
        b.set_param("ohx_colsample_bynode", "0")
    rc, msg = c_call(b, name, nfeat)
    assert rc == -1 and "OHXBoosterBoostTreesSampled" in msg
    for k in NAMES:
        b.set_param(k, "1.0")
    rc, msg = c_call(b, name, nfeat)
    assert rc == -1 and "OHXBoosterBoostTreesSampled" not in msg and "DMatrix" in msg, msg
    assert saved(b) == before
    b.free()


def test_the_abi_is_what_it_was():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    names = re.findall(r"^(?:int|const char\*|void)\s+((?:XG|OHX)\w+)\(", header, re.M)
    assert sorted(names) == sorted(capi.ABI_SYMBOLS) and len(names) == 78
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    for hidden in ("ohx_grow_colsample", "grow_colsample_splits", "grow_pick_level_features", "GrowColsample"):
        assert hidden not in nm and hidden not in " ".join(capi.ABI_SYMBOLS), hidden
    exported = [ln.split()[-1] for ln in nm.splitlines() if ln.split()[-2] not in "WwVvu" and not ln.split()[-1].startswith("__hip_cuid_")]
    assert sorted(exported) == sorted(capi.ABI_SYMBOLS), "no new symbol"
    for name in NAMES:
        assert header.index('"' + name + '"') < header.index("int XGBoosterSetParam(")
    for said in ("K_lvl(i, d) = mix(K_col(i) + gamma64 * (d + 1))", "K_node(i, p) = mix(K_col(i) + gamma64 * (32 + p))",
                 "n_lvl = max(1, (int) floor((double)colsample_bylevel * n_sel))", "n_node = max(1, (int) floor((double)colsample_bynode * n_lvl))",
                 "C1.", "C2.", "C3."):
        assert said in header, said


# ---- the host exports against the restatement ----

def test_the_keys():
    for seed in SEEDS:
        for i in TREES:
            for d in LEVELS:
                for p in NODES:
                    assert synth.colsample_keys(seed, i, d, p) == (int(K.level_key(seed, i, d)), int(K.node_key(seed, i, p))), (seed, i, d, p)
    # a level key and a node key never share an input: d + 1 <= 18 < 32 <= 32 + p
    assert max(d + 1 for d in range(18)) < K.NODE_KEY_BASE
    assert len({synth.colsample_keys(3, 1, d, p)[k] for d in range(18) for p in range(64) for k in (0, 1)}) == 18 + 64


def test_the_counts():
    assert K.count(F32(0.34), 3) == 1 and K.count(F32(0.99), 1) == 1 and K.count(F32(1.0), 128) == 128
    assert K.count(2.0 ** -20, 128) == 1 and K.count(0.5, 27) == 13 and K.count(0.3, 128) == 38 and K.count(0.5, 128) == 64
    assert K.draws_nothing(1, 0.99, 0.99) and K.draws_nothing(3, 1.0, 1.0) and not K.draws_nothing(3, 0.99, 1.0)
    for n in LISTS:
        for fr in FRACTIONS:
            lst = np.arange(n, dtype=np.uint8)
            assert len(synth.boost_level_features(1, 0, 0, lst, fr)) == K.count(fr, n) == len(synth.boost_node_features(1, 0, 0, lst, fr))


def tree_lists(rng, n):
    """Lists of n features: the first n, and n of 128 drawn, ascending."""
    yield list(range(n))
    yield sorted(int(f) for f in rng.choice(128, n, replace=False))


def test_level_and_node_lists_against_the_restatement_and_the_rank():
    rng = np.random.default_rng(2900)
    drawn = 0
    for n in LISTS:
        for lst in tree_lists(rng, n):
            for fr in FRACTIONS:
                seed, i = SEEDS[int(rng.integers(len(SEEDS)))], TREES[int(rng.integers(len(TREES)))]
                for d in LEVELS:
                    lvl = synth.boost_level_features(seed, i, d, lst, fr).tolist()
                    assert lvl == K.level_features(seed, i, d, lst, fr), (seed, i, d, n, fr)
                    assert set(lvl) <= set(lst) and lvl == sorted(lvl), "nested in the tree's list, ascending"
                    if len(lvl) == n:
                        assert lvl == lst, "n_lvl == n_sel draws nothing"
                    for p in NODES[:2] + NODES[3:] if d else NODES[:1]:
                        for fn in (0.5, fr):
                            mine = synth.boost_node_features(seed, i, p, lvl, fn).tolist()
                            assert mine == K.node_features(seed, i, p, lvl, fn), (seed, i, p, n, fr, fn)
                            assert set(mine) <= set(lvl) and mine == sorted(mine), "nested in the level's list, ascending"
                            # the rank the kernels compute names the same set
                            ranked = [f for f in lvl if synth.boost_node_has_feature(seed, i, p, lvl, len(mine), f)]
                            assert ranked == mine, (seed, i, p, lvl, mine, ranked)
                            drawn += len(mine) < len(lvl)
    assert drawn > 300
    # the draw moves with the seed, the tree, the level and the node
    lst = list(range(27))
    base = K.level_features(7, 2, 3, lst, 0.5)
    assert base != K.level_features(8, 2, 3, lst, 0.5) and base != K.level_features(7, 3, 3, lst, 0.5) and base != K.level_features(7, 2, 4, lst, 0.5)
    assert K.node_features(7, 2, 5, base, 0.5) != K.node_features(7, 2, 6, base, 0.5)


def test_key_ties_go_to_the_smaller_feature():
    """Equal keys cannot be asked of mix, so the tie is put into the restatement's and the library's shared order by
    hand: (key, f) with equal keys orders by f, in the sort and in the rank."""
    assert K.smallest([5, 5, 5, 1], [9, 3, 7, 11], 2) == [3, 11] and K.smallest([5, 5, 5], [9, 3, 7], 1) == [3]
    assert K.smallest([2, 2], [0, 1], 1) == [0] and K.smallest([2, 1], [0, 1], 1) == [1]
    # the library's comparison is the one function grow_draw_below, which the host check program asks with equal keys


def test_inclusion_frequencies_at_13_of_27():
    """Every feature of a level's 27 is in S_node for about 13/27 of 2^14 node ids: within 5 sigma of the binomial."""
    lvl = list(range(27))
    n = 1 << 14
    hits = np.zeros(27, dtype=np.int64)
    for p in range(n):
        mine = synth.boost_node_features(42, 1, p, lvl, 0.5)
        assert len(mine) == 13
        hits[mine] += 1
    q = 13.0 / 27.0
    sigma = math.sqrt(n * q * (1.0 - q))
    assert hits.sum() == 13 * n and np.all(np.abs(hits - n * q) <= 5.0 * sigma), (hits.tolist(), n * q, sigma)
    for p in (0, 1, 77, 9999):        # the restatement stays inside the host function
        assert synth.boost_node_features(42, 1, p, lvl, 0.5).tolist() == K.node_features(42, 1, p, lvl, 0.5)


# ---- a case worked by hand ----

HAND_X = np.array([[0, 0], [1, 1], [2, 0], [3, 1], [4, 0], [5, 1], [6, 0], [7, 1]], F32)
HAND_Y = np.array([4, 5, 4, 5, 0, 1, 0, 1], F32) + F32(K.BASE)


def hand_case(bylevel, bynode, seed):
    cuts = G.quantile_cuts(HAND_X, float("nan"), 64)
    return K.boost(bylevel, bynode, (), "squarederror", 1.0, 0.0, 0.0, "rmse", np.full(8, K.BASE, F32), HAND_X, float("nan"), HAND_Y, None,
                   cuts, 2, rounds=1, max_depth=2, eta=0.5, lam=0.0, gamma=0.0, min_child_weight=0.0, seed=seed)


def test_a_case_worked_by_hand():
    """The eight rows of tests/test_grow_mono_cpu.py: free, the root splits on x0 < 4 with loss_chg 32 and both children on
    x1 with loss_chg 1.  With colsample_bylevel = 0.5 every level sees one of the two features.  Where level 0 draws x1
    the root splits on x1 < 1 (8^2 / 4 + 12^2 / 4 - 50 = 2, weights 2 and 3); a child then holds x0 = 0 2 4 6 (or 1 3 5 7)
    with y - 0.5 = 4 4 0 0 (5 5 1 1): if level 1 draws x0 it splits between 2 and 4 (3 and 5), at the cut 3 (4), with
    8^2 / 2 + 0 - 8^2 / 4 = 16 (10^2 / 2 + 2^2 / 2 - 12^2 / 4 = 16); if it draws x1 again, which holds one value there, nothing splits."""
    want = {}
    for seed in range(64):
        lv = tuple(K.level_features(seed, 0, d, [0, 1], 0.5)[0] for d in (0, 1))
        want.setdefault(lv, seed)
    assert len(want) == 4, "all four pairs of draws come up among 64 seeds"
    t = hand_case(0.5, 1.0, want[1, 0])["trees"][0]
    assert t["left"].tolist() == [1, 3, 5, -1, -1, -1, -1] and t["feature"][:3].tolist() == [1, 0, 0]
    assert t["loss_chg"][:3].tolist() == [2.0, 16.0, 16.0] and t["base_weight"].tolist() == [2.5, 2.0, 3.0, 4.0, 0.0, 5.0, 1.0]
    assert t["value"][:3].tolist() == [1.0, 3.0, 4.0], "of two cuts that part the rows alike the smaller j is taken"
    t = hand_case(0.5, 1.0, want[1, 1])["trees"][0]
    assert t["left"].tolist() == [1, -1, -1] and t["feature"].tolist() == [1, 0, 0] and t["loss_chg"].tolist() == [2.0, 0.0, 0.0]
    t = hand_case(0.5, 1.0, want[0, 1])["trees"][0]
    assert t["left"].tolist() == [1, 3, 5, -1, -1, -1, -1] and t["feature"][:3].tolist() == [0, 1, 1], "the free tree"
    assert t["loss_chg"][:3].tolist() == [32.0, 1.0, 1.0]
    t = hand_case(0.5, 1.0, want[0, 0])["trees"][0]
    assert t["feature"][:3].tolist() == [0, 0, 0] and t["loss_chg"][0] == 32.0, "x0 alone: the children split on x0 again"
    # by node: the same four outcomes of a node's own draw, and the log says which node was narrowed
    out = hand_case(1.0, 0.5, 5)
    for e in out["draws"][0]:
        assert len(e["node"]) == 1 and e["level"] == [0, 1] and e["node"] == K.node_features(5, 0, e["p"], [0, 1], 0.5)
        assert e["feature"] is None or e["feature"] in e["node"]
    # fractions that take nothing away are the other restatement's call
    assert hand_case(1.0, 1.0, 3)["draws"] is None and hand_case(0.99, 0.99, 3)["draws"] is not None


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_colsample.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_colsample.hip")
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
def test_colsample_kernels_resources_and_atomics(isa, kernel):
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
    assert _figure(report, kernel, "VGPRs") <= 128 and _figure(report, kernel, "Occupancy [waves/SIMD]") >= 4
    if re.search(r"[a-z]ELi(\d)E", kernel).group(1) == "0":      # phase 0: the rank is a ballot and a population count, two keys a lane
        assert "s_bcnt1_i32_b64" in body and "v_cmp" in body


def test_the_file_holds_its_own_kernels_and_reuses_the_rest(isa):
    text, _ = isa
    symbols = re.findall(r"^(_Z\w+):\s*; @\1$", text, re.M)
    for k in KERNELS:
        assert len([s for s in symbols if k in s]) == 1, k
    assert len(symbols) == len(KERNELS) == 18
    csrc = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    src = open(os.path.join(csrc, "grow_colsample.hip")).read()
    assert "grow_split_columns(" in src and "grow_split_nodes<" in src and "grow_deep_split_chunks(" in src
    for own in ("__shfl", "r.base_weight", "hipMemsetAsync", "hipStreamSynchronize", "for (uint32_t c0", "Ghist", "bins[", "hipFuncSetAttribute",
                "grow_gain", "loss_chg"):
        assert own not in src, own
    assert "-ffp-contract=off" in re.search(r"grow_colsample_kernels\.o:.*\n\t.*", open(os.path.join(csrc, "Makefile")).read()).group(0)


# ---- the host functions under sanitizers ----

def test_the_draws_under_sanitizers(tmp_path):
    """tools/grow_colsample_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_colsample_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_colsample_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert re.search(r"\d+ lists, \d+ ranks, 0 failures", r.stdout), r.stdout
