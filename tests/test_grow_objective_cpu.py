"""The boosting objectives ("ohx_objective"), what can be checked without a GPU: the library's own pair (csrc/grow.hpp
grow_pair, reached through libohx_synth.so's ohx_grow_pairs) against the restatement written from the header, bit for bit,
over random and crafted residuals, weights and slopes, with its flags; at squared error the pairs of the weighted call;
the three parameters' refusals, which need no device; the ABI unchanged; the new kernels cross-compiled for gfx950 with no
scratch, no spill, no float atomic, no compare-and-swap and correctly rounded float32 divisions in the pair kernel; and the
plan with the pair planes under sanitizers in a program of its own."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_objective_support as O
from tests import grow_weighted_support as W
from tests import helpers
from tests.test_grow_cpu import kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
SLOPES = (2.0 ** -10, 0.5, 1.0, 3.7, 256.0)
WEIGHTS = np.asarray((0.0, 2.0 ** -24, 1.0, 255.99), np.float32)
KERNELS = ["grow_pair_kernelILj0E", "grow_pair_kernelILj1E", "grow_hist_pairs_kernel", "grow_deep_hist_pairs_kernel",
           "grow_split_pairs_kernelILi0ELi0E", "grow_split_pairs_kernelILi1ELi0E", "grow_split_pairs_kernelILi1ELi1E",
           "grow_split_pairs_kernelILi1ELi2E"]
F32 = np.float32


def restated_or_flags(objective, slope, pred, y, w):
    """The restatement row by row: (q, hq, flags) with a refused row's pair (0, 0), as the library hands them out."""
    n = len(y)
    q, hq, flags = np.zeros(n, np.int64), np.zeros(n, np.uint64), 0
    try:
        return (*O.pairs(objective, slope, pred, y, w), 0)
    except ValueError:
        pass
    for r in range(n):
        try:
            a, b = O.pairs(objective, slope, pred[r:r + 1], y[r:r + 1], None if w is None else w[r:r + 1])
            q[r], hq[r] = a[0], b[0]
        except ValueError as e:
            flags |= synth.GROW_FLAG_LABEL if str(e).startswith("label") else synth.GROW_FLAG_WEIGHT
    return q, hq, flags


def same_pairs(objective, slope, pred, y, w, what):
    q, hq, flags = restated_or_flags(objective, slope, pred, y, w)
    gq, gh, gflags = synth.ohx_grow_pairs(objective, slope, pred, y, w)
    assert gflags == flags, (what, gflags, flags)
    bad = np.flatnonzero((gq != q) | (gh.astype(np.uint64) != hq))
    assert bad.size == 0, (what, bad[:6], gq[bad[:6]], q[bad[:6]], gh[bad[:6]], hq[bad[:6]])
    return q, hq


# ---- the pair against the restatement ----

@pytest.mark.parametrize("slope", SLOPES)
def test_random_residuals_bit_for_bit(slope):
    rng = np.random.default_rng(2600)
    n = 200000
    # residuals of every size from 2^-45 to just below 256, either sign
    z = (rng.choice((-1.0, 1.0), n) * np.exp2(rng.uniform(-45.0, 7.99, n))).astype(F32)
    y = rng.standard_normal(n).astype(F32)
    pred = (y + z).astype(F32)
    keep = np.abs(pred - y) < F32(255.0)
    pred, y = pred[keep], y[keep]
    w = rng.choice(np.asarray((0.0, 2.0 ** -24, 0.25, 0.5, 1.0), F32), len(y))     # |g| <= |z| < 256: no |gw| refusal
    for objective in O.OBJECTIVES:
        q, hq = same_pairs(objective, slope, pred, y, w, f"{objective} at {slope}")
        same_pairs(objective, slope, pred, y, None, f"{objective} at {slope}, no weights")
        # (two weights in five and the residuals below 2^-25 give q = 0: the inputs are not mostly zeros)
        assert np.count_nonzero(q) > len(y) // 5
    if slope <= 1.0:
        assert len(np.unique(hq)) > 10000, "pseudo-Huber hessians are no row weights"


@pytest.mark.parametrize("slope", SLOPES)
def test_crafted_residuals_and_weights_bit_for_bit(slope):
    below = np.nextafter(F32(256.0), F32(0.0))
    zs = np.asarray([0.0, -0.0, 2.0 ** -70, -2.0 ** -70, 2.0 ** -149, -2.0 ** -149, 2.0 ** -130, 3e-39, 2.0 ** -126, -2.0 ** -126,
                     2.0 ** -24, 2.0 ** -25, 0.5, 1.0, -3.7, 16.0, 200.0, -200.5, 255.0, below, -below], F32)
    z = np.repeat(zs, len(WEIGHTS))
    w = np.tile(WEIGHTS, len(zs))
    pred, y = z.copy(), np.zeros(len(z), F32)             # pred - 0 is z itself
    for objective in O.OBJECTIVES:
        q, hq, flags = restated_or_flags(objective, slope, pred, y, w)
        gq, gh, gflags = synth.ohx_grow_pairs(objective, slope, pred, y, w)
        assert gflags == flags and np.array_equal(gq, q) and np.array_equal(gh.astype(np.uint64), hq), (objective, slope)
        tiny = np.abs(z) < F32(2.0 ** -126)
        assert not gq[tiny].any(), "a denormal residual gives q = 0"
        assert not gq[w == 0].any() and not gh[w == 0].any()
        if objective == "squarederror":
            # |gw| >= 256 at the heaviest weight: "label", and the row's pair is (0, 0)
            heavy = (np.abs(z) * w >= 256.0)
            assert heavy.any() and (flags & synth.GROW_FLAG_LABEL) and not gq[heavy].any() and not gh[heavy].any()


def test_hessians_that_round_to_zero():
    """h < 2^-25 gives hq = 0 while the gradient stays: far residuals at the smallest slope, and at any slope under a
    weight of 2^-24."""
    z = np.asarray([150.0, 200.0, -200.5, 255.0], F32)
    q, hq = same_pairs("pseudohuber", 2.0 ** -10, z, np.zeros(4, F32), np.ones(4, F32), "far residuals")
    g, h = O.pair_floats("pseudohuber", 2.0 ** -10, z)
    assert np.all(h < F32(2.0 ** -25)) and not hq.any() and np.all(q != 0)
    q, hq = same_pairs("pseudohuber", 1.0, z, np.zeros(4, F32), np.full(4, 2.0 ** -24, F32), "a weight of one unit")
    assert not hq.any() and np.all(np.abs(q) == 1)


def test_flags():
    y = np.zeros(8, F32)
    pred = np.asarray([1.0, np.nan, 256.0, -300.0, np.inf, 2.0, 2.0, 200.0], F32)
    for objective in O.OBJECTIVES:
        q, hq, flags = synth.ohx_grow_pairs(objective, 1.0, pred, y, None)
        assert flags == synth.GROW_FLAG_LABEL and q[0] != 0 and not q[1:5].any() and not hq[1:5].any() and q[5] != 0
        for bad in (np.nan, -1.0, 256.0, np.inf, -np.inf):
            w = np.ones(8, F32)
            w[5] = bad
            q, hq, flags = synth.ohx_grow_pairs(objective, 1.0, pred, y, w)
            assert flags == (synth.GROW_FLAG_LABEL | synth.GROW_FLAG_WEIGHT) and q[5] == 0 and hq[5] == 0 and q[6] != 0
        # a NaN label under a bad weight says "label": the residual is looked at before the weight
        q, hq, flags = synth.ohx_grow_pairs(objective, 1.0, np.asarray([np.nan], F32), y[:1], np.asarray([-1.0], F32))
        assert flags == synth.GROW_FLAG_LABEL
    # |gw| >= 256: squared error reaches it, pseudo-Huber's |g| < delta cannot at slope 1
    w = np.full(8, 2.0, F32)
    ok = np.asarray([1.0, 2.0, 3.0, 4.0, 5.0, 2.0, 2.0, 200.0], F32)
    assert synth.ohx_grow_pairs("squarederror", 1.0, ok, y, w)[2] == synth.GROW_FLAG_LABEL
    assert synth.ohx_grow_pairs("pseudohuber", 1.0, ok, y, w)[2] == 0
    for slope in (0.0, 2.0 ** -11, 257.0, np.nan):
        with pytest.raises(capi.OhxError, match="slope"):
            synth.ohx_grow_pairs("pseudohuber", slope, ok, y, w)


def test_squared_error_pairs_are_the_weighted_calls():
    rng = np.random.default_rng(2601)
    n = 50000
    y = rng.standard_normal(n).astype(F32)
    pred = (y + 4.0 * rng.standard_normal(n)).astype(F32)
    w = rng.choice(np.arange(0.0, 4.25, 0.25).astype(F32), n)
    q, hq, flags = synth.ohx_grow_pairs("squarederror", 1.0, pred, y, w)
    assert flags == 0
    assert np.array_equal(q, W.grad_fixed(W.residuals(pred, y), w)) and np.array_equal(hq.astype(np.uint64), W.hess_fixed(w))


def test_the_pair_planes_in_the_plan():
    for n in (1, 4097, 55987200, 1 << 31):
        for depth in (1, 8, 12, 18):
            p = synth.grow_pairs_plan(n, 27, 27 * 254, depth, 256)
            assert p == {"pairs_bytes": 12 * n, "row_bytes": 12}


# ---- the parameters, which need no device ----

def test_the_three_parameters_and_their_refusals():
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    for good in (("ohx_objective", "squarederror"), ("ohx_objective", "pseudohuber"), ("ohx_huber_slope", "0.0009765625"),
                 ("ohx_huber_slope", "256"), ("ohx_huber_slope", "3.7"), ("ohx_huber_slope", "1e-2"), ("ohx_grow_pairs", "on"),
                 ("ohx_grow_pairs", "auto"), ("objective", "reg:anything")):
        b.set_param(*good)
    for name, values in (("ohx_objective", ("", "huber", "reg:pseudohubererror", "PSEUDOHUBER", "logistic")),
                         ("ohx_huber_slope", ("0", "nan", repr(2.0 ** -11), "257", "text", "", "1x", "-1", "inf", "1 ")),
                         ("ohx_grow_pairs", ("off", "", "1"))):
        for v in values:
            with pytest.raises(capi.OhxError, match=name):
                b.set_param(name, v)
    assert saved(b) == before, "no parameter is written into a model"
    b.free()


def test_the_abi_is_what_it_was():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    assert "ohx_grow_pairs" not in capi.ABI_SYMBOLS
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    assert "ohx_grow_pairs" not in nm and "grow_pair" not in nm, "the pair is test support, not the product's ABI"
    for name in ("ohx_objective", "ohx_huber_slope", "ohx_grow_pairs"):
        assert header.index('"' + name + '"') < header.index("int XGBoosterSetParam(")
    assert "s = sqrtf(1.0f + z2 / d2)" in header and "denormal" in header


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_pairs.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_pairs.hip")
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
def test_pair_kernels_resources_and_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    assert _figure(report, kernel, "VGPRs Spill") == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    vgprs, occupancy = _figure(report, kernel, "VGPRs"), _figure(report, kernel, "Occupancy [waves/SIMD]")
    if "hist" in kernel:
        assert "v_div" not in body and "v_sqrt" not in body and "v_rndne" not in body, "a histogram kernel computes no gradient"
        assert vgprs <= 64 and occupancy == 8, (vgprs, occupancy)
        adds = [l for l in body.splitlines() if "global_atomic_add_x2" in l]
        assert not any("sc0" in l for l in adds), "the global adds return nothing"
        assert "s_load_dwordx2" in body, "the bag's word by a scalar load"
        if "deep" in kernel:
            assert len(adds) == 2 * 32 and "ds_" not in body and _figure(report, kernel, "LDS Size [bytes/block]") == 0
        else:
            assert len(adds) == 2 and len(re.findall(r"ds_add_u64", body)) >= 2 and "ds_add_u32" not in body
    elif "grow_pair_kernel" in kernel:
        assert "atomic_add" not in body and "ds_" not in body
        assert vgprs <= 64 and occupancy == 8, (vgprs, occupancy)
        assert len(re.findall(r"global_store_dwordx2", body)) >= 1 and len(re.findall(r"global_store_dword\b", body)) >= 1
        if "ILj1E" in kernel:
            # three float32 divisions, each the correctly rounded sequence, never a bare reciprocal; and a square root
            for op in ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32"):
                assert len(re.findall(op, body)) >= 3, op
            assert len(re.findall(r"v_rcp_f32", body)) == len(re.findall(r"v_div_fmas_f32", body)), "a reciprocal only inside a division"
            assert "v_sqrt_f32" in body and "v_rsq_f32" not in body
        else:
            assert "v_div" not in body and "v_rcp" not in body and "v_sqrt" not in body, "squared error divides nothing"
    else:
        assert "atomic_add" not in body and "ds_add" not in body
        assert vgprs <= 128 and occupancy >= 4, (vgprs, occupancy)
        if "ILi0E" in kernel:
            assert "v_div_scale_f64" in body, "the gain divides in double"


def test_the_file_holds_its_own_kernels_and_the_others_are_what_they_were(isa):
    text, _ = isa
    symbols = re.findall(r"^(_Z\w+):\s*; @\1$", text, re.M)
    for k in KERNELS:
        assert len([s for s in symbols if k in s]) == 1, k
    assert len(symbols) == len(KERNELS)
    csrc = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    src = open(os.path.join(csrc, "grow_pairs.hip")).read()
    # the split phases and the level loop are grow_device.hpp's; the deep level loop is grow_deep.hip's
    assert "grow_split_columns(" in src and "grow_split_nodes<" in src and "grow_launch_tree(" in src
    assert "launch_grow_tree_deep_with(" in src
    for own in ("grow_best_split", "__shfl_up", "r.base_weight", "a.max_depth; ++d", "hipMemsetAsync", "hipStreamSynchronize"):
        assert own not in src, own
    assert "-ffp-contract=off" in re.search(r"grow_pairs_kernels\.o:.*\n\t.*", open(os.path.join(csrc, "Makefile")).read()).group(0)


# ---- the plan and the pair under sanitizers ----

def test_the_plan_and_the_pair_under_sanitizers(tmp_path):
    """tools/grow_pairs_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_pairs_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_pairs_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert re.search(r"\d+ plans, \d+ pairs, 0 failures", r.stdout), r.stdout
