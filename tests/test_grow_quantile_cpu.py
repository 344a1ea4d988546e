"""Quantile boosting ("ohx_objective" = quantile, "ohx_quantile_alpha", "ohx_eval_metric" = quantile), what can be checked
without a GPU: the parameters and their refusals; the ABI unchanged; the header's key lines; the library's own pair
(csrc/grow.hpp grow_pair<kGrowObjQuantile>, through libohx_synth.so) against the restatement written from the header, bit
for bit; the host build of the per-leaf select and of one pick (csrc/grow_quantile.hpp) against a sort, and against the
coverage property checked on its own; the pinball sums and the reported value against Python integers; the new kernels
cross-compiled for gfx950 with no scratch, no spill, no float atomic and no compare-and-swap; and the shared host/device
functions under sanitizers in a program of its own."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_quantile_support as Q
from tests import grow_weighted_support as W
from tests import helpers
from tests.test_grow_cpu import kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
WEIGHTS = np.asarray((0.0, 2.0 ** -24, 1.0, 255.99), F32)
KERNELS = ["grow_pair_quantile_kernel", "grow_quantile_slots_kernel", "grow_quantile_pass_kernel", "grow_quantile_pick_kernel",
           "grow_sse_quantile_kernel", "grow_walk_sse_quantile_kernel", "grow_deep_walk_sse_quantile_kernel"]


# ---- the parameters, which need no device ----

def test_the_objective_is_accepted():
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    b.set_param("ohx_objective", "quantile")
    b.set_param("ohx_eval_metric", "quantile")
    b.set_param("ohx_objective", "squarederror")
    b.free()


def test_quantile_alpha_values_and_refusals():
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    for good in ("0.5", "0.0009765625", "0.9990234375", "0.05", "0.95", "5e-2", repr(2.0 ** -10), repr(1.0 - 2.0 ** -10)):
        b.set_param("ohx_quantile_alpha", good)
    for bad in ("", "0", "1", "nan", "1x", "0.5 ", "-0.1", "inf", repr(2.0 ** -11), repr(1.0 - 2.0 ** -11), "half"):
        with pytest.raises(capi.OhxError, match="ohx_quantile_alpha"):
            b.set_param("ohx_quantile_alpha", bad)
    for name, values in (("ohx_objective", ("", "QUANTILE", "reg:quantileerror", "logistic")),
                         ("ohx_eval_metric", ("", "pinball", "logloss", "Quantile"))):
        for v in values:
            with pytest.raises(capi.OhxError, match=name):
                b.set_param(name, v)
    b.set_param("quantile_alpha", "7")            # the names without the prefix stay ignored
    b.set_param("objective", "reg:quantileerror")
    assert saved(b) == before, "no parameter is written into a model"
    b.free()


def test_the_abi_is_what_it_was():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    names = re.findall(r"^(?:int|const char\*|void)\s+((?:XG|OHX)\w+)\(", header, re.M)
    assert sorted(names) == sorted(capi.ABI_SYMBOLS) and len(names) == 78
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    for hidden in ("ohx_grow_quantile", "grow_quantile", "launch_grow_tree_quantile", "ohx_grow_weighted_quantile"):
        assert hidden not in nm and hidden not in " ".join(capi.ABI_SYMBOLS), hidden
    exported = [ln.split()[-1] for ln in nm.splitlines() if ln.split()[-2] not in "WwVvu" and not ln.split()[-1].startswith("__hip_cuid_")]
    assert sorted(exported) == sorted(capi.ABI_SYMBOLS), "no new symbol"


def test_the_header_holds_the_definition():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    for name in ("ohx_quantile_alpha", "ohx_objective", "ohx_eval_metric"):
        assert header.index('"' + name + '"') < header.index("int XGBoosterSetParam(")
    for line in ("alpha_q = (uint32) rint(alpha * 2^24)", "g = (z >= 0) ? 1.0f - alpha : -alpha; h = 1.0f",
                 "k*  = the smallest key with alpha_q * W_p <= 2^24 * C_p(k*)", "value = q_p * eta",
                 "sq = |e| * (z < 0 ? alpha_q : 2^24 - alpha_q)", "((double)S_t * 2^-72) / ((double)W * 2^-24)",
                 "-0.0f counts as +0.0f", "no interpolation", "squarederror (default) | pseudohuber | quantile",
                 "rmse (default) | mae | pseudohuber | quantile"):
        assert line in header, line


# ---- the pair against the restatement ----

def restated_or_flags(alpha, pred, y, w):
    n = len(y)
    q, hq, flags = np.zeros(n, np.int64), np.zeros(n, np.uint64), 0
    try:
        return (*Q.pairs(alpha, pred, y, w), 0)
    except ValueError:
        pass
    for r in range(n):
        try:
            a, b = Q.pairs(alpha, pred[r:r + 1], y[r:r + 1], None if w is None else w[r:r + 1])
            q[r], hq[r] = a[0], b[0]
        except ValueError as e:
            flags |= synth.GROW_FLAG_LABEL if str(e).startswith("label") else synth.GROW_FLAG_WEIGHT
    return q, hq, flags


@pytest.mark.parametrize("alpha", Q.ALPHAS)
def test_crafted_residuals_and_weights_bit_for_bit(alpha):
    below = Q.BELOW_256
    zs = np.asarray([0.0, -0.0, 2.0 ** -70, -2.0 ** -70, 2.0 ** -149, -2.0 ** -149, 2.0 ** -130, 3e-39, 2.0 ** -126, -2.0 ** -126,
                     2.0 ** -24, 2.0 ** -25, 0.5, 1.0, -3.7, 16.0, 200.0, -200.5, 255.0, below, -below, 256.0, np.nan], F32)
    z = np.repeat(zs, len(WEIGHTS))
    w = np.tile(WEIGHTS, len(zs))
    pred, y = z.copy(), np.zeros(len(z), F32)             # pred - 0 is z itself
    for wt in (w, None):
        q, hq, flags = restated_or_flags(alpha, pred, y, wt)
        gq, gh, gflags = synth.ohx_grow_pairs("quantile", alpha, pred, y, wt)
        assert gflags == flags == synth.GROW_FLAG_LABEL, "256 and NaN are refused"
        assert np.array_equal(gq, q) and np.array_equal(gh.astype(np.uint64), hq), alpha
        sound = np.abs(z) < F32(256.0)
        aq = Q.alpha_q(alpha)
        if wt is None:
            assert np.all(gq[sound & (z >= 0)] == Q.ONE - aq) and np.all(gq[sound & (z < 0)] == -aq), "-0.0 counts as z >= 0"
            assert np.all(gh[sound] == Q.ONE) and not gq[~sound].any() and not gh[~sound].any()
        else:
            assert not gq[w == 0].any() and not gh[w == 0].any()
            assert np.array_equal(gh[sound].astype(np.uint64), W.hess_fixed(w[sound]))


def test_random_residuals_bit_for_bit_and_bad_alphas():
    rng = np.random.default_rng(3201)
    n = 100000
    y = rng.standard_normal(n).astype(F32)
    pred = (y + (rng.choice((-1.0, 1.0), n) * np.exp2(rng.uniform(-45.0, 7.9, n)))).astype(F32)
    w = rng.choice(np.asarray((0.0, 2.0 ** -24, 0.25, 1.0, 200.0), F32), n)
    for alpha in Q.ALPHAS:
        q, hq, flags = restated_or_flags(alpha, pred, y, w)
        gq, gh, gflags = synth.ohx_grow_pairs("quantile", alpha, pred, y, w)
        assert gflags == flags and np.array_equal(gq, q) and np.array_equal(gh.astype(np.uint64), hq), alpha
    for alpha in (0.0, 1.0, 2.0 ** -11, np.nan):
        with pytest.raises(capi.OhxError, match="alpha"):
            synth.ohx_grow_pairs("quantile", alpha, pred[:4], y[:4], None)


# ---- the select against the restatement, and against the property ----

def select_case(leaves):
    """The crafted leaves as the rows of nodes 1, 2, .. of one tree -> (pos, hq, pred, y, node ids)."""
    pos = np.concatenate([np.full(len(r), i + 1, np.uint16) for i, (_, r, _) in enumerate(leaves)])
    y = np.concatenate([r for _, r, _ in leaves])
    hq = W.hess_fixed(np.concatenate([w for _, _, w in leaves]))
    return pos, hq, np.zeros(len(y), F32), y, np.arange(1, len(leaves) + 1, dtype=np.uint16)


@pytest.mark.parametrize("alpha", Q.ALPHAS)
def test_the_host_select_on_crafted_leaves(alpha):
    leaves = Q.crafted_leaves()
    pos, hq, pred, y, ids = select_case(leaves)
    found, key, value, Wl = synth.grow_quantile_leaves(pos, hq, pred, y, ids, alpha, eta=0.125)
    aq = Q.alpha_q(alpha)
    k = Q.keys(y)
    for s, (name, r, w) in enumerate(leaves):
        rows = pos == ids[s]
        want = Q.leaf_key(k[rows], hq[rows], aq)
        assert int(Wl[s]) == int(hq[rows].astype(object).sum()), name
        if want is None:
            assert not found[s] and name == "every row weighs 0", name
            continue
        assert found[s] and int(key[s]) == want, (name, alpha, hex(int(key[s])), hex(want))
        assert helpers.bits(value[s:s + 1])[0] == helpers.bits(np.asarray([Q.leaf_value(want, 0.125)], F32))[0], name
        assert Q.covers(k[rows], hq[rows], aq, int(key[s])), (name, "the property")
        assert Q.leaf_key_fast(k[rows], hq[rows], aq) == want
    # -0.0 counts as +0.0: the leaf of zeros is +0.0 whatever the sign bits say
    zeros = [n for n, _, _ in leaves].index("+0.0 against -0.0")
    if 0.2 < alpha < 0.8:
        assert int(key[zeros]) == 0x80000000 and helpers.bits(value[zeros:zeros + 1])[0] == 0


def test_the_host_select_on_many_rows_and_leaves():
    """2^16 rows of random keys and weights in one leaf, and 256 leaves of random sizes beside it."""
    rng = np.random.default_rng(3202)
    n = 1 << 16
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    r = bits.view(F32).copy()
    r[~(np.abs(r) < F32(256.0))] = F32(0.25)                 # (NaN fails the comparison)
    w = rng.choice(np.asarray((0.0, 2.0 ** -24, 0.5, 1.0, 3.0, Q.BELOW_256), F32), n)
    hq = W.hess_fixed(w)
    k = Q.keys(r)
    for alpha in Q.ALPHAS:
        aq = Q.alpha_q(alpha)
        found, key, value, Wl = synth.grow_quantile_leaves(np.full(n, 7, np.uint16), hq, np.zeros(n, F32), r, [7], alpha)
        assert found[0] and int(key[0]) == Q.leaf_key_fast(k, hq, aq) and Q.covers(k, hq, aq, int(key[0]))
        assert helpers.bits(value)[0] == helpers.bits(np.asarray([Q.unkey(int(key[0]))], F32))[0]
    pos = rng.integers(0, 300, n).astype(np.uint16)          # nodes 256 .. 299 are no leaves of the call
    ids = np.arange(256, dtype=np.uint16)[::-1].copy()       # slots in another order than the nodes
    resid = (rng.standard_normal(n) * 3.0).astype(F32)
    pred = rng.standard_normal(n).astype(F32)
    y = (pred + resid).astype(F32)
    k = Q.keys(y - pred)
    found, key, value, Wl = synth.grow_quantile_leaves(pos, hq, pred, y, ids, 0.95, eta=0.5)
    aq = Q.alpha_q(0.95)
    for s, p in enumerate(ids):
        rows = pos == p
        assert found[s] and int(key[s]) == Q.leaf_key_fast(k[rows], hq[rows], aq) and Q.covers(k[rows], hq[rows], aq, int(key[s])), p


def test_one_pick_over_a_leafs_bins():
    bins = np.zeros(256, np.uint64)
    assert synth.grow_quantile_pick(bins, 0, 0.5) is None, "no weight, no pick"
    bins[[3, 200, 255]] = (10, 20, 70)
    assert synth.grow_quantile_pick(bins, 0, 0.05) == (3, 0, 100)
    assert synth.grow_quantile_pick(bins, 0, 0.5) == (255, 30, 100)
    bins[:] = 0
    bins[[0, 9]] = (5, 65)
    # a later pass (its bins sum to the weight of the digit picked before): the prefix grows by the digit, `below` by the
    # bins beneath it; alpha_q * 100 <= 2^24 * (30 + 5) fails at 0.5 and holds at 0.25
    assert synth.grow_quantile_pick(bins, 1, 0.5, prefix=255, below=30, W=100) == ((255 << 8) | 9, 35, 100)
    assert synth.grow_quantile_pick(bins, 1, 0.25, prefix=255, below=30, W=100) == ((255 << 8) | 0, 30, 100)
    # exact at the boundary: alpha = 0.5 and half the weight below or at the digit holds the rule with equality
    bins[:] = 0
    bins[[1, 2]] = (1 << 62, 1 << 62)
    assert synth.grow_quantile_pick(bins, 0, 0.5)[0] == 1
    bins[1] -= 1
    assert synth.grow_quantile_pick(bins, 0, 0.5)[0] == 2, "one unit short of half, at sums near 2^63"


# ---- the launch shape of the pass kernel ----

def test_the_plan_of_the_pass_kernel():
    """synth.grow_quantile_plan is the function launch_grow_tree_quantile calls (csrc/grow_quantile.hpp plan_grow_quantile).
    The figures below are worked out by hand from its text: a block holds min(64, 2^depth) leaves, and the blocks over the
    rows are row_blocks / (8 * groups), at least one and no more than the rows need at 1024 a block."""
    for depth in range(1, 9):
        assert synth.grow_quantile_plan(1, depth, 256) == dict(pass_blocks=1, pass_block_rows=1024, group=min(64, 1 << depth),
                                                               groups=(1, 1, 1, 1, 1, 1, 2, 4)[depth - 1], row_blocks=1), depth
    # 4097 rows are 17 blocks of 256 and 5 of 1024: 17 // 8 = 2 of them with one group, 17 // 16 = 1 with two, 17 // 32 = 0 -> 1
    for depth, group, groups, blocks in ((1, 2, 1, 2), (6, 64, 1, 2), (7, 64, 2, 1), (8, 64, 4, 1)):
        assert synth.grow_quantile_plan(4097, depth, 256) == dict(pass_blocks=blocks, pass_block_rows=1024, group=group, groups=groups,
                                                                  row_blocks=17), depth
    # 2^31 rows on 256 CUs: 2048 row blocks, a block a CU over all groups
    for depth, blocks in ((1, 256), (6, 256), (7, 128), (8, 64)):
        p = synth.grow_quantile_plan(1 << 31, depth, 256)
        assert (p["pass_blocks"], p["row_blocks"]) == (blocks, 2048) and p["pass_blocks"] * p["groups"] == 256, depth
    for cus in (1, 2, 7, 8, 64, 104, 256, 304):
        for nrow in (1, 63, 1024, 1025, 4097, 262144, 262145, 528450, 55987200, 1 << 31):
            rows = synth.grow_plan_weighted(nrow, 3, 0, 6, cus)["row_blocks"]
            assert rows == synth.grow_plan(nrow, 3, 0, 6, cus)["row_blocks"], "the row blocks do not depend on the histograms' bins"
            for depth in range(1, 9):
                p = synth.grow_quantile_plan(nrow, depth, cus)
                assert p["pass_blocks"] >= 1 and p["groups"] * p["group"] >= 1 << depth, (cus, nrow, depth)
                assert p["group"] <= 64 and p["groups"] * p["group"] < (1 << depth) + p["group"], "no empty group"
                assert p["row_blocks"] == rows and p["pass_block_rows"] == 1024
                assert p["pass_blocks"] == max(1, min((nrow + 1023) // 1024, rows // (8 * p["groups"]))), (cus, nrow, depth)
    for bad in (dict(nrow=0, max_depth=6), dict(nrow=4097, max_depth=0), dict(nrow=4097, max_depth=9)):
        with pytest.raises(Exception, match="ohx_grow_quantile_plan"):
            synth.grow_quantile_plan(num_cus=256, **bad)


# ---- the metric ----

def test_the_pinball_term_the_sums_and_the_reported_value():
    rng = np.random.default_rng(3203)
    n = 50000
    y = rng.standard_normal(n).astype(F32)
    pred = (y + (rng.choice((-1.0, 1.0), n) * np.exp2(rng.uniform(-30.0, 7.9, n)))).astype(F32)
    pred[:4], y[:4] = (0.0, -0.0, 255.0, -255.0), 0.0
    w = rng.choice(np.asarray((0.0, 2.0 ** -24, 1.0, Q.BELOW_256), F32), n)
    hq = W.hess_fixed(w)
    for alpha in Q.ALPHAS:
        sq, sound = synth.ohx_grow_metric_row("quantile", alpha, pred, y)
        want = Q.pinball_terms(alpha, W.residuals(pred, y))
        assert sound.all() and [int(v) for v in sq] == list(want), alpha
        assert max(want) < 1 << 56
        S, Wsum = Q.metric_sum("quantile", 1.0, alpha, W.residuals(pred, y), hq), int(hq.astype(object).sum())
        assert S > 1 << 64, "beyond one word"
        got = synth.boost_weighted_quantile(S >> 64, (S >> 32) & 0xFFFFFFFF, S & 0xFFFFFFFF, Wsum)
        assert got == Q.metric_value("quantile", S, Wsum), alpha
        # the mean pinball loss, near enough in floating point
        z = (pred.astype(np.float64) - y.astype(np.float64))
        a = float(F32(alpha))
        loss = np.where(z < 0, a * -z, (1.0 - a) * z)
        assert abs(got - float((loss * w).sum() / w.sum())) < 1e-5 * max(1.0, got)
    bad = synth.ohx_grow_metric_row("quantile", 0.5, np.asarray([256.0, np.nan, 1.0], F32), np.zeros(3, F32))
    assert bad[1].tolist() == [False, False, True] and not bad[0][:2].any()
    with pytest.raises(capi.OhxError, match="alpha"):
        synth.ohx_grow_metric_row("quantile", 1.0, pred[:2], y[:2])


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_quantile.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_quantile.hip")
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
def test_quantile_kernels_resources_and_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    assert _figure(report, kernel, "VGPRs Spill") == 0 and _figure(report, kernel, "SGPRs Spill") == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    assert "v_div" not in body and "v_rcp" not in body and "v_sqrt" not in body and "v_rsq" not in body, "nothing divides"
    vgprs, occupancy = _figure(report, kernel, "VGPRs"), _figure(report, kernel, "Occupancy [waves/SIMD]")
    assert vgprs <= 64 and occupancy == 8, (vgprs, occupancy)
    adds = [l for l in body.splitlines() if "global_atomic_add_x2" in l]
    assert not any("sc0" in l for l in adds), "the global adds return nothing"
    if kernel == "grow_quantile_pass_kernel":
        assert len(adds) == 1 and len(re.findall(r"ds_add_u64", body)) == 1 and "ds_add_rtn" not in body
    elif kernel in ("grow_pair_quantile_kernel", "grow_quantile_slots_kernel", "grow_quantile_pick_kernel"):
        assert not adds and "ds_add" not in body
    else:
        assert len(adds) in (3, 4), "p2, p1, p0 (and W)"


def test_the_file_holds_its_own_kernels_and_reuses_the_rest(isa):
    text, _ = isa
    symbols = re.findall(r"^(_Z\w+):\s*; @\1$", text, re.M)
    for k in KERNELS:
        assert len([s for s in symbols if k in s]) == 1, k
    assert len(symbols) == len(KERNELS)
    csrc = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    src = open(os.path.join(csrc, "grow_quantile.hip")).read()
    # the levels are the pair path's, the leaf kernel grow.hip's, the rule grow_quantile.hpp's
    assert "launch_grow_levels_pairs(" in src and "launch_grow_leaf(" in src and "grow_quantile_reached(" in src
    assert "grow_walk_row(" in src and "grow_stage_tree(" in src and "grow_reduce_wide(" in src
    for own in ("grow_best_split", "grow_split_columns(", "hipStreamSynchronize", "atomicCAS", "__int128"):
        assert own not in src, own
    assert "-ffp-contract=off" in re.search(r"grow_quantile_kernels\.o:.*\n\t.*", open(os.path.join(csrc, "Makefile")).read()).group(0)


# ---- the shared functions under sanitizers ----

def test_the_select_the_pair_and_the_term_under_sanitizers(tmp_path):
    """tools/grow_quantile_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_quantile_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_quantile_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert re.search(r"\d+ selects, \d+ rows, 0 failures", r.stdout), r.stdout
