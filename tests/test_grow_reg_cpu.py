""""ohx_reg_alpha", "ohx_max_delta_step" and "ohx_eval_metric", what can be checked without a GPU: the library's own policy
(csrc/grow.hpp GrowRegHess, reached through libohx_synth.so's ohx_grow_reg_gain / ohx_grow_reg_leaf) and a row's term of each
metric (ohx_grow_metric_row) against the restatement written from the header, bit for bit, over random and crafted sums and
residuals; at alpha = m = 0 the bits of today's gain and leaf; a node's split over the policy; the three parameters and
their refusals, which need no device; the ABI unchanged; the new kernels cross-compiled for gfx950 with no scratch, no
spill, no flat access, no float atomic, the gain's double division and the metric kernels' division and square-root
counts; and the policy and the metric row under sanitizers in a program of its own."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_reg_support as RG
from tests import grow_weighted_support as W
from tests import helpers
from tests.test_grow_cpu import kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
ONE = 1 << 24
SPLIT_KERNELS = ["grow_split_reg_kernelILi0ELi0E", "grow_split_reg_kernelILi1ELi0E", "grow_split_reg_kernelILi1ELi1E",
                 "grow_split_reg_kernelILi1ELi2E", "grow_deep_split_reg_kernelILi0E", "grow_deep_split_reg_kernelILi1E"]
METRIC_KERNELS = [k + m for k in ("grow_sse_metric_kernel", "grow_walk_sse_metric_kernel", "grow_deep_walk_sse_metric_kernel")
                  for m in ("ILj1E", "ILj2E")]
KERNELS = SPLIT_KERNELS + METRIC_KERNELS
ALPHAS = (0.0, 0.5, 2.0, 1e6)
STEPS = (0.0, 0.25, 0.5, 1.0)
LAMBDAS = (0.0, 1.0, 2.5)


def bits(v):
    return np.asarray(v, F32).view(np.uint32).tolist()


def dbits(v):
    return np.asarray(v, np.float64).view(np.uint64).tolist()


def same_policy(Gs, H, lam, alpha, m, eta=0.125):
    got = synth.ohx_grow_reg_gain(Gs, H, lam, alpha, m)
    want = RG.gain(Gs, H, lam, alpha, m)
    assert dbits(got) == dbits(want), ("gain", Gs, H, lam, alpha, m, got, want)
    leaf = synth.ohx_grow_reg_leaf(Gs, H, eta, lam, alpha, m)
    assert bits(leaf) == bits(RG.solve(Gs, H, eta, lam, alpha, m)), ("leaf", Gs, H, lam, alpha, m)
    return got, leaf


# ---- the policy against the restatement ----

def test_random_sums_bit_for_bit():
    rng = np.random.default_rng(2700)
    clipped = zeroed = 0
    for _ in range(20000):
        Gs = int(rng.integers(-(1 << 34), 1 << 34)) >> int(rng.integers(0, 30))
        H = int(rng.integers(1, 1 << 36)) >> int(rng.integers(0, 30)) or 1
        lam, alpha, m = float(rng.choice(LAMBDAS)), float(rng.choice(ALPHAS)), float(rng.choice(STEPS))
        _, (leaf, w, sh) = same_policy(Gs, H, lam, alpha, m)
        clipped += m > 0 and abs(w) == F32(m)
        zeroed += Gs != 0 and w == 0
    assert clipped > 1000 and zeroed > 1000, "the sums reach both rules"


def test_crafted_sums_bit_for_bit():
    sums = [0, 1, -1, ONE // 2, -ONE // 2, ONE, -ONE, ONE + 1, -ONE - 1, ONE - 1, 3 * ONE, -3 * ONE, (1 << 40) - 1, -(1 << 40) + 1]
    for Gs in sums:
        for H in (1, ONE // 2, ONE, 7 * ONE, 1 << 40):
            for lam in LAMBDAS:
                for alpha in ALPHAS + (1.0,):
                    for m in STEPS:
                        gain, (leaf, w, sh) = same_policy(Gs, H, lam, alpha, m)
                        Gd = float(Gs) * 2.0 ** -24
                        if abs(Gd) <= alpha:          # G = 0, |Gd| = alpha exactly, alpha far above every |Gd|
                            assert bits(w) == bits(-0.0) and gain == 0.0, (Gs, H, alpha, m)
                        if m > 0:
                            assert abs(w) <= F32(m)
    # |w| = m exactly: Gd = -1, D = 2 gives 0.5, which is not clipped, and one unit more of G is clipped to the same bits
    for Gs, what in ((-ONE, "exact"), (-ONE - 1, "clipped")):
        _, (leaf, w, sh) = same_policy(Gs, ONE, 1.0, 0.0, 0.5, eta=1.0)
        assert w == F32(0.5), what
    assert same_policy(-ONE + 1, ONE, 1.0, 0.0, 0.5)[1][1] < F32(0.5)


def test_at_the_defaults_the_bits_are_the_weighted_calls():
    rng = np.random.default_rng(2701)
    cases = [(0, 1), (0, ONE), (1, 1), (-1, ONE)] + [(int(rng.integers(-(1 << 40), 1 << 40)), int(rng.integers(1, 1 << 40)))
                                                     for _ in range(5000)]
    for Gs, H in cases:
        for lam in (0.0, 1.0):
            leaf = synth.ohx_grow_reg_leaf(Gs, H, 0.3, lam, 0.0, 0.0)
            assert bits(leaf) == bits(synth.grow_solve_leaf_weighted(Gs, H, 0.3, lam)), (Gs, H, lam)
            assert bits(leaf) == bits(W.solve(Gs, H, 0.3, lam))
            assert dbits(synth.ohx_grow_reg_gain(Gs, H, lam, 0.0, 0.0)) == dbits(W.gain(Gs, H, lam)), (Gs, H, lam)
    assert bits(synth.ohx_grow_reg_leaf(0, ONE, 0.3, 1.0, 0.0, 0.0)[1]) == bits(-0.0), "a base_weight of -0.0f at G == 0"


def test_a_nodes_split_over_the_policy():
    """grow_node_split with GrowRegHess against grow_weighted_support.best_split run with the restated gain."""
    rng = np.random.default_rng(2702)
    F = 3
    ncuts = [254, 7, 1]
    cut_ptr = np.concatenate(([0], np.cumsum(ncuts)))
    for case in range(40):
        Gh = np.zeros((F, 256), np.int64)
        Hh = np.zeros((F, 256), np.uint64)
        n = 400
        q = (rng.standard_normal(n) * 2.0 ** 24 * (8.0 if case % 2 else 0.3)).astype(np.int64)
        hq = rng.integers(0, 3 * ONE, n).astype(np.uint64)
        for f in range(F):
            b = np.where(rng.random(n) < 0.1, 255, rng.integers(0, ncuts[f] + 1, n))
            np.add.at(Gh[f], b, q)
            np.add.at(Hh[f], b, hq)
        Gp, Hp = int(q.sum()), int(hq.astype(object).sum())
        for alpha, m in ((0.0, 0.0), (0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (2.0, 1.0), (1e6, 0.0)):
            for mcw in (0.0, 30.0):
                g = dict(W.__dict__)
                g["gain"] = lambda Gs, H, lam, a=alpha, s=m: RG.gain(Gs, H, lam, a, s)
                want = types.FunctionType(W.best_split.__code__, g)(Gh, Hh, ncuts, Gp, Hp, 1.0, mcw)
                got = synth.grow_reg_node_split(Gh, Hh, cut_ptr, Gp, Hp, 1.0, mcw, alpha, m)
                assert (got is None) == (want is None), (case, alpha, m, mcw)
                if got is not None:
                    assert dbits(got[0]) == dbits(want[0]) and got[1:] == tuple(int(v) for v in want[1:]), (case, alpha, m, got, want)


# ---- the metric row against the restatement ----

@pytest.mark.parametrize("metric", RG.METRICS)
def test_the_metric_row_bit_for_bit(metric):
    rng = np.random.default_rng(2703)
    n = 200000
    z = (rng.choice((-1.0, 1.0), n) * np.exp2(rng.uniform(-80.0, 7.99, n))).astype(F32)
    below = np.nextafter(F32(256.0), F32(0.0))
    crafted = np.asarray([0.0, -0.0, 2.0 ** -70, -2.0 ** -70, 2.0 ** -149, -2.0 ** -149, 2.0 ** -130, 3e-39, 2.0 ** -126, -2.0 ** -126,
                          2.0 ** -64, 2.0 ** -63, 2.0 ** -25, 2.0 ** -24, 0.5, 1.0, -3.7, 16.0, 200.0, -200.5, 255.0, below, -below], F32)
    z = np.concatenate((crafted, z))
    zero = np.zeros(len(z), F32)                       # pred - 0 is z itself
    for slope in (2.0 ** -10, 0.5, 1.0, 3.7, 256.0):
        sq, sound = synth.ohx_grow_metric_row(metric, slope, z, zero)
        want = RG.metric_terms(metric, slope, z)
        assert sound.all()
        bad = [i for i in range(len(z)) if int(sq[i]) != int(want[i])]
        assert not bad, (metric, slope, bad[:5], z[bad[:5]], sq[bad[:5]], want[bad[:5]])
        tiny = np.abs(z) < F32(2.0 ** -70)
        assert not sq[tiny].any(), "zero and denormal residuals add nothing"
        assert int(sq.max()) < {"rmse": 1 << 64, "mae": 1 << 32, "pseudohuber": 1 << 40}[metric]
        if metric != "pseudohuber":
            break                                      # (the slope is not read)
    # refused residuals: sq = 0 and the row is not sound
    bad = np.asarray([np.nan, 256.0, -300.0, np.inf, -np.inf], F32)
    sq, sound = synth.ohx_grow_metric_row(metric, 1.0, bad, np.zeros(5, F32))
    assert not sound.any() and not sq.any()
    # the sum and its value: Python ints, then the header's conversion
    hq = W.hess_fixed(rng.choice(np.arange(0.0, 2.5, 0.5).astype(F32), 5000))
    S, Wsum = RG.metric_sum(metric, 1.0, z[:5000], hq), int(hq.astype(object).sum())
    p2, p1, p0 = S >> 64, (S >> 32) & 0xFFFFFFFF, S & 0xFFFFFFFF
    value = synth.boost_weighted_rmse(p2, p1, p0, Wsum) if metric == "rmse" else synth.boost_weighted_mean(p2, p1, p0, Wsum)
    assert value == RG.metric_value(metric, S, Wsum)


def test_pseudohuber_terms_are_what_the_formula_says():
    z = np.asarray([1e-3, 0.5, 1.0, 3.7, 100.0, 255.0], F32)
    for slope in (0.5, 1.0, 3.7):
        got = np.asarray([int(v) for v in RG.metric_terms("pseudohuber", slope, z)], np.float64) * 2.0 ** -24
        zd = z.astype(np.float64)
        exact = slope * slope * (np.sqrt(1.0 + zd * zd / (slope * slope)) - 1.0)
        assert np.all(np.abs(got - exact) <= 1e-6 * exact + 2.0 ** -24), (slope, got, exact)


# ---- the parameters, which need no device ----

def test_the_three_parameters_and_their_refusals():
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    for good in (("ohx_reg_alpha", "0"), ("ohx_reg_alpha", "0.5"), ("ohx_reg_alpha", "1e3"), ("ohx_max_delta_step", "0"),
                 ("ohx_max_delta_step", "0.7"), ("ohx_max_delta_step", "1e-2"), ("ohx_eval_metric", "rmse"), ("ohx_eval_metric", "mae"),
                 ("ohx_eval_metric", "pseudohuber"), ("reg_alpha", "anything"), ("max_delta_step", "anything"), ("eval_metric", "auc")):
        b.set_param(*good)
    for name in ("ohx_reg_alpha", "ohx_max_delta_step"):
        for v in ("", "1x", "1 ", "nan", "inf", "-inf", "-1", "-0.5", "text"):
            with pytest.raises(capi.OhxError, match=name):
                b.set_param(name, v)
    for v in ("", "RMSE", "mse", "huber", "mae ", "logloss"):
        with pytest.raises(capi.OhxError, match="ohx_eval_metric"):
            b.set_param("ohx_eval_metric", v)
    with pytest.raises(capi.OhxError, match="ohx_objective"):
        b.set_param("ohx_objective", "logistic")
    assert saved(b) == before, "no parameter is written into a model"
    b.free()


def test_the_abi_is_what_it_was():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    names = re.findall(r"^(?:int|const char\*|void)\s+((?:XG|OHX)\w+)\(", header, re.M)
    assert sorted(names) == sorted(capi.ABI_SYMBOLS) and len(names) == 78
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    for hidden in ("ohx_grow_reg", "ohx_grow_metric", "grow_reg_splits", "launch_grow_sse_metric"):
        assert hidden not in nm and hidden not in " ".join(capi.ABI_SYMBOLS), hidden
    exported = [ln.split()[-1] for ln in nm.splitlines() if ln.split()[-2] not in "WwVvu" and not ln.split()[-1].startswith("__hip_cuid_")]
    assert sorted(exported) == sorted(capi.ABI_SYMBOLS), "no new symbol"
    for name in ("ohx_reg_alpha", "ohx_max_delta_step", "ohx_eval_metric"):
        assert header.index('"' + name + '"') < header.index("int XGBoosterSetParam(")
    assert "ThresholdL1" in header and "copysign(m, w)" in header and "mf = z2 / (1.0f + s)" in header and "-0.0f" in header
    assert "CalcGain" in header and "2^-48" in header


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_reg.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_reg.hip")
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
def test_reg_kernels_resources_divisions_and_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    assert _figure(report, kernel, "VGPRs Spill") == 0 and _figure(report, kernel, "SGPRs Spill") == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    assert "v_fma_mix" not in body and "v_rsq" not in body
    vgprs, occupancy = _figure(report, kernel, "VGPRs"), _figure(report, kernel, "Occupancy [waves/SIMD]")
    count = lambda op: len(re.findall(op, body))
    if kernel in SPLIT_KERNELS:
        assert "atomic_add" not in body and "ds_add" not in body
        assert vgprs <= 128 and occupancy >= 4, (vgprs, occupancy)
        # the gain (phase 0) and the leaf (phase 1) divide in double by the correctly rounded sequence, never a bare reciprocal
        assert count("v_div_scale_f64") >= 2 and count("v_div_fmas_f64") >= 1 and count("v_div_fixup_f64") >= 1
        assert count("v_rcp_f64") == count("v_div_fmas_f64"), "a reciprocal only inside a division"
        assert "v_rcp_f32" not in body and "v_div_scale_f32" not in body
    else:
        assert vgprs <= 64 and occupancy == 8, (vgprs, occupancy)
        adds = [l for l in body.splitlines() if "global_atomic_add_x2" in l]
        assert len(adds) in (3, 4) and not any("sc0" in l for l in adds), "p2, p1, p0 (and W) leave by integer adds that return nothing"
        assert "v_div_scale_f64" not in body and "v_rcp_f64" not in body and "v_sqrt_f64" not in body
        if "ILj2E" in kernel:
            # two correctly rounded float32 divisions and a square root with its correction
            assert count("v_div_fmas_f32") == 2 and count("v_div_fixup_f32") == 2 and count("v_div_scale_f32") == 4
            assert count("v_rcp_f32") == 2, "a reciprocal only inside a division"
            assert count("v_sqrt_f32") == 1
        else:
            assert "v_div" not in body and "v_rcp" not in body and "v_sqrt" not in body, "mae divides nothing"
        lds = _figure(report, kernel, "LDS Size [bytes/block]")
        if "grow_walk_sse_metric" in kernel:
            assert lds >= 512 * 16, "the tree is staged in LDS"
        else:
            assert lds < 512


def test_the_file_holds_its_own_kernels_and_reuses_the_rest(isa):
    text, _ = isa
    symbols = re.findall(r"^(_Z\w+):\s*; @\1$", text, re.M)
    for k in KERNELS:
        assert len([s for s in symbols if k in s]) == 1, k
    assert len(symbols) == len(KERNELS)
    csrc = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    src = open(os.path.join(csrc, "grow_reg.hip")).read()
    # the split phases, the chunk loop, the walk and the reduction are the shared headers'; no histogram, pair, bin,
    # partition, leaf, widen or stage kernel is written again
    assert "grow_split_columns(" in src and "grow_split_nodes<" in src and "grow_deep_split_chunks(" in src
    assert "grow_walk_row(" in src and "grow_stage_tree(" in src and "grow_reduce_wide(" in src and "launch_grow_deep_stage(" in src
    for own in ("grow_best_split", "__shfl", "r.base_weight", "hipMemsetAsync", "hipStreamSynchronize", "for (uint32_t c0", "Ghist",
                "bins[", "hipFuncSetAttribute"):
        assert own not in src, own
    assert "-ffp-contract=off" in re.search(r"grow_reg_kernels\.o:.*\n\t.*", open(os.path.join(csrc, "Makefile")).read()).group(0)
    deep = open(os.path.join(csrc, "grow_deep_device.hpp")).read()
    assert len(re.findall(r"for \(uint32_t c0 = 0;", deep)) == 1 and "template <class Hess>" in deep


# ---- the policy and the metric row under sanitizers ----

def test_the_policy_and_the_metric_row_under_sanitizers(tmp_path):
    """tools/grow_reg_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_reg_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_reg_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert re.search(r"\d+ sums, \d+ rows, 0 failures", r.stdout), r.stdout
