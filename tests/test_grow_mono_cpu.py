""""ohx_monotone_constraints" without a GPU (csrc/grow.hpp GrowMonoHess, the constrained grow_best_split,
grow_mono_node_split; the parameter's grammar in csrc/capi.cpp): the host exports against the restatement
(tests/grow_mono_support.py) bit for bit, a case worked by hand, the inputs of the GPU property test run through the
restatement, the cross-compiled kernels' resources, and the host code under AddressSanitizer and UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_mono_support as M
from tests import grow_reg_support as RG
from tests import grow_support as G
from tests import helpers
from tests.test_grow_cpu import kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
F32 = np.float32
ONE = 1 << 24
INF = float("inf")
NAME = "ohx_monotone_constraints"
KERNELS = ["grow_split_mono_kernelILi0ELi0E", "grow_split_mono_kernelILi1ELi0E", "grow_split_mono_kernelILi1ELi1E",
           "grow_split_mono_kernelILi1ELi2E", "grow_deep_split_mono_kernelILi0E", "grow_deep_split_mono_kernelILi1E"]
# (lo, hi): the whole line, a half line either way, intervals around and beside 0, and an interval of one point
INTERVALS = ((-INF, INF), (-INF, -0.25), (0.25, INF), (-0.5, 0.5), (0.0, INF), (-INF, -0.0), (0.0, 0.0), (0.125, 0.125), (-2.0, -1.0))


def bits(v):
    return np.asarray(v, F32).view(np.uint32).tolist()


def dbits(v):
    return np.asarray(v, np.float64).view(np.uint64).tolist()


# ---- the parameter, which needs no device ----

GOOD = ("()", "( )", "(1)", "(0)", "(-1)", "(+1)", "(1,0,-1)", "(1, 0, -1)", " (\t1 ,+1,\t-1 ) ", str((1, 0, -1)), str((-1, 1)), "(0,0,0)",
        "(" + ",".join(["1", "0", "-1", "+1"] * 32) + ")")
# (str((1,)) is "(1,)": a trailing comma, which the header refuses; the binding writes a sequence out itself)
BAD = ("", " ", "1", "1,0", "(1", "1)", "(2)", "(1.0)", "(-0)", "(+0)", "(1,)", "(,1)", "(,)", "(1,,0)", "(1 0)", "(- 1)", "(+)", "(a)", "(1)x",
       "((1))", "[1,0]", "(10)", "(1;0)", "(" + ",".join(["0"] * 129) + ")", "(" + ",".join(["1"] * 129) + ")")


def test_the_grammar_of_the_parameter():
    assert len(M.parse(GOOD[-1])) == 128
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    for v in GOOD:
        M.parse(v)                                     # the restatement reads the header's grammar the same way
        b.set_param(NAME, v)
    b.set_param("monotone_constraints", "anything")    # the name without the prefix stays accepted and ignored
    for v in BAD:
        with pytest.raises(ValueError):
            M.parse(v)
        with pytest.raises(capi.OhxError, match=NAME):
            b.set_param(NAME, v)
    assert saved(b) == before, "the parameter is written into no model"
    b.free()


def test_the_abi_is_what_it_was():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    names = re.findall(r"^(?:int|const char\*|void)\s+((?:XG|OHX)\w+)\(", header, re.M)
    assert sorted(names) == sorted(capi.ABI_SYMBOLS) and len(names) == 78
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    for hidden in ("ohx_grow_mono", "grow_mono_splits", "GrowMono"):
        assert hidden not in nm and hidden not in " ".join(capi.ABI_SYMBOLS), hidden
    assert header.index('"' + NAME + '"') < header.index("int XGBoosterSetParam(")
    for said in ("gain_w(G, H, w)", "w < lo ? lo : (w > hi ? hi : w)", "mid = (wL + wR) * 0.5", "non-decreasing", "default_left"):
        assert said in header, said


# ---- the host exports against the restatement ----

def same_policy(Gs, H, lam, alpha, m, lo, hi, eta=0.125):
    w = synth.ohx_grow_mono_weight(Gs, H, lam, alpha, m, lo, hi)
    want = M.weight(Gs, H, lam, alpha, m, lo, hi)
    assert dbits(w) == dbits(want), ("weight", Gs, H, lam, alpha, m, lo, hi, w, want)
    gain = synth.ohx_grow_mono_gain(Gs, H, lam, alpha, w)
    assert dbits(gain) == dbits(M.gain_w(Gs, H, lam, alpha, want)), ("gain_w", Gs, H, lam, alpha, w)
    leaf = synth.ohx_grow_mono_leaf(Gs, H, eta, lam, alpha, m, lo, hi)
    assert bits(leaf) == bits(M.solve(Gs, H, eta, lam, alpha, m, lo, hi)), ("leaf", Gs, H, lam, alpha, m, lo, hi)
    return w, gain, leaf


def test_random_sums_bit_for_bit():
    rng = np.random.default_rng(2800)
    low = high = inside = 0
    for _ in range(20000):
        Gs = int(rng.integers(-(1 << 34), 1 << 34)) >> int(rng.integers(0, 30))
        H = int(rng.integers(1, 1 << 36)) >> int(rng.integers(0, 30)) or 1
        lam, alpha, m = float(rng.choice((0.0, 1.0, 2.5))), float(rng.choice((0.0, 0.5, 2.0))), float(rng.choice((0.0, 0.5, 1.0)))
        lo, hi = INTERVALS[int(rng.integers(len(INTERVALS)))]
        if rng.random() < 0.5:
            lo, hi = sorted(float(v) for v in rng.standard_normal(2))
        w, _, _ = same_policy(Gs, H, lam, alpha, m, lo, hi)
        free = synth.ohx_grow_mono_weight(Gs, H, lam, alpha, m, -INF, INF)
        low += free < lo
        high += free > hi
        inside += lo <= free <= hi
        assert lo <= w <= hi
    assert min(low, high, inside) > 1000, "the sums reach both ends and the inside"


def test_crafted_sums_bit_for_bit():
    sums = [0, 1, -1, ONE // 2, -ONE // 2, ONE, -ONE, ONE + 1, 3 * ONE, -3 * ONE, (1 << 40) - 1, -(1 << 40) + 1]
    for Gs in sums:
        for H in (1, ONE, 7 * ONE, 1 << 40):
            for alpha, m in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)):
                for lo, hi in INTERVALS:
                    w, gain, (leaf, bw, sh) = same_policy(Gs, H, 1.0, alpha, m, lo, hi)
                    assert lo <= w <= hi
                    if lo == hi:
                        assert w == lo, "an interval of one point"
    # -0.0: G = 0 gives -0.0, which is not below an interval that starts at +0.0, so it stays; its base_weight is -0.0f
    for lo, hi in ((-INF, INF), (0.0, INF), (-0.0, 1.0), (-1.0, 0.0)):
        w, _, (leaf, bw, _) = same_policy(0, ONE, 1.0, 0.0, 0.0, lo, hi)
        assert dbits(w) == dbits(-0.0) and bits(bw) == bits(-0.0), (lo, hi)
    # clamped at either end to the end's own bits: Gd = -1, D = 2 gives 0.5
    assert dbits(same_policy(-ONE, ONE, 1.0, 0.0, 0.0, -INF, 0.25)[0]) == dbits(0.25)
    assert dbits(same_policy(-ONE, ONE, 1.0, 0.0, 0.0, 0.75, INF)[0]) == dbits(0.75)
    assert dbits(same_policy(-ONE, ONE, 1.0, 0.0, 0.0, 0.5, 0.5)[0]) == dbits(0.5)
    assert dbits(same_policy(-ONE, ONE, 1.0, 0.0, 0.0, -0.0, 0.0)[0]) == dbits(0.0)        # w > hi: hi as it is written
    # the step clips before the interval clamps: m = 0.25 gives 0.25, which an interval above it moves again
    assert dbits(same_policy(-ONE, ONE, 1.0, 0.0, 0.25, -INF, INF)[0]) == dbits(0.25)
    assert dbits(same_policy(-ONE, ONE, 1.0, 0.0, 0.25, 0.375, INF)[0]) == dbits(0.375)


def test_on_the_whole_line_under_a_step_the_policy_is_the_regularised_one():
    rng = np.random.default_rng(2801)
    for _ in range(3000):
        Gs, H = int(rng.integers(-(1 << 40), 1 << 40)), int(rng.integers(1, 1 << 40))
        for alpha, m in ((0.0, 0.5), (0.5, 0.5), (2.0, 1.0)):
            w = synth.ohx_grow_mono_weight(Gs, H, 1.0, alpha, m, -INF, INF)
            assert dbits(synth.ohx_grow_mono_gain(Gs, H, 1.0, alpha, w)) == dbits(synth.ohx_grow_reg_gain(Gs, H, 1.0, alpha, m))
            assert bits(synth.ohx_grow_mono_leaf(Gs, H, 0.3, 1.0, alpha, m, -INF, INF)) == bits(synth.ohx_grow_reg_leaf(Gs, H, 0.3, 1.0, alpha, m))


def histograms(rng, ncuts, n, scale):
    F = len(ncuts)
    Gh, Hh = np.zeros((F, 256), np.int64), np.zeros((F, 256), np.uint64)
    q = (rng.standard_normal(n) * 2.0 ** 24 * scale).astype(np.int64)
    hq = rng.integers(0, 3 * ONE, n).astype(np.uint64)
    for f in range(F):
        b = np.where(rng.random(n) < 0.1, 255, rng.integers(0, ncuts[f] + 1, n))
        np.add.at(Gh[f], b, q)
        np.add.at(Hh[f], b, hq)
    return Gh, Hh, int(q.sum()), int(hq.astype(object).sum())


def test_a_nodes_split_under_constraints():
    """grow_mono_node_split against the restated best_split and children: the winner, its loss_chg and both intervals."""
    rng = np.random.default_rng(2802)
    ncuts = [60, 7, 1]
    cut_ptr = np.concatenate(([0], np.cumsum(ncuts)))
    moved = refused = 0
    for case in range(24):
        Gh, Hh, Gp, Hp = histograms(rng, ncuts, 400, 8.0 if case % 2 else 0.3)
        for cons in ((1, 0, 0), (-1, 0, 0), (1, -1, 1), (0, 0, -1), (0, 0, 0)):
            for alpha, m in ((0.0, 0.0), (0.5, 0.5)):
                for lo, hi in ((-INF, INF), (-0.05, 0.05), (0.01, INF), (0.02, 0.02)):
                    for mcw in (0.0, 30.0, 400.0):       # (the node holds about 600: the last looks at no candidate)
                        want = M.best_split(Gh, Hh, ncuts, Gp, Hp, 1.0, mcw, alpha, m, lo, hi, cons)
                        got = synth.grow_mono_node_split(Gh, Hh, cut_ptr, Gp, Hp, 1.0, mcw, alpha, m, lo, hi, cons)
                        assert (got is None) == (want is None), (case, cons, alpha, m, lo, hi, mcw)
                        refused += got is None
                        if got is None:
                            continue
                        assert dbits(got[0]) == dbits(want[0]) and got[1:6] == tuple(int(v) for v in want[1:6]), (case, cons, got, want)
                        (loL, hiL), (loR, hiR) = M.children(cons[want[1]], want[6], want[7], lo, hi)
                        assert dbits(got[6]) == dbits((loL, hiL, loR, hiR)), (case, cons, got, want)
                        free = M.best_split(Gh, Hh, ncuts, Gp, Hp, 1.0, mcw, alpha, m, lo, hi, (0, 0, 0))
                        moved += free[1:4] != want[1:4]
    assert moved > 20 and refused > 0, (moved, refused)
    # wL == wR is in order for either direction: two children with the same sums, and an interval of one point
    Gh, Hh = np.zeros((1, 256), np.int64), np.zeros((1, 256), np.uint64)
    Gh[0, :2], Hh[0, :2] = (-ONE, -ONE), (ONE, ONE)
    for c in (1, -1):
        got = synth.grow_mono_node_split(Gh, Hh, [0, 1], -2 * ONE, 2 * ONE, 1.0, 0.0, 0.0, 0.0, -INF, INF, (c,))
        assert got is not None and got[1:4] == (0, 0, 0) and got[6] == ((-INF, 0.5, 0.5, INF) if c > 0 else (0.5, INF, -INF, 0.5)), (c, got)
    Gh[0, :2] = (-3 * ONE, ONE)
    for c in (1, -1):
        got = synth.grow_mono_node_split(Gh, Hh, [0, 1], -2 * ONE, 2 * ONE, 1.0, 0.0, 0.0, 0.0, 0.25, 0.25, (c,))
        assert got is not None and got[6] == (0.25, 0.25, 0.25, 0.25), (c, got)


# ---- a case worked by hand ----

HAND_X = np.array([[0, 0], [1, 1], [2, 0], [3, 1], [4, 0], [5, 1], [6, 0], [7, 1]], F32)
HAND_Y = np.array([4, 5, 4, 5, 0, 1, 0, 1], F32) + F32(M.BASE)


def hand_case(constraints):
    cuts = G.quantile_cuts(HAND_X, float("nan"), 64)
    assert cuts[0].tolist() == [0, 7, 8] and cuts[1].tolist() == [1, 2, 3, 4, 5, 6, 7, 1]
    return cuts, M.boost(constraints, "squarederror", 1.0, 0.0, 0.0, "rmse", np.full(8, M.BASE, F32), HAND_X, float("nan"), HAND_Y, None,
                         cuts, 2, rounds=1, max_depth=2, eta=0.5, lam=0.0, gamma=0.0, min_child_weight=0.0)


def test_a_case_worked_by_hand():
    """8 rows of weight 1, pred = 0.5 and y - 0.5 = 4 5 4 5 0 1 0 1, so g = -(y - 0.5); lambda = 0, eta = 0.5; x0 = 0 .. 7,
    x1 = 0 1 0 1 ...  A node's weight is the mean of its y - 0.5 and its gain G^2 / H (gain_w at that weight is the same
    number: -(2 G w + H w^2) with w = -G / H).

    Free: the root splits on x0 < 4 (left 18^2 / 4 = 81, right 2^2 / 4 = 1, parent 20^2 / 8 = 50: loss_chg 32; x1 gives
    8^2 / 4 + 12^2 / 4 - 50 = 2), and both children split on x1 (32 + 50 - 81 = 1 and 0 + 2 - 1 = 1): seven nodes.
    With c_0 = +1 every cut of x0 has the larger mean on its left (4 > 16/7, 4.5 > 11/6, 13/3 > 7/5, 4.5 > 0.5, 3.6 > 2/3,
    19/6 > 0.5, 19/7 > 1), so no candidate on x0 is admitted: the root splits on x1 < 1 with loss_chg 2, weights 2 and 3.
    Its children hold one value of x1 each and every cut of x0 is still out of order: three nodes.
    With c_0 = -1 the free tree is in order; the root's mid is (4.5 + 0.5) / 2 = 2.5, the left child's interval
    (2.5, +inf) holds its children's 4 and 5, the right child's (-inf, 2.5) its 0 and 1: the free tree's numbers."""
    _, free = hand_case(())
    t = free["trees"][0]
    assert t["left"].tolist() == [1, 3, 5, -1, -1, -1, -1] and t["feature"][:3].tolist() == [0, 1, 1]
    assert t["value"].tolist() == [4.0, 1.0, 1.0, 2.0, 2.5, 0.0, 0.5] and t["loss_chg"][:3].tolist() == [32.0, 1.0, 1.0]
    _, up = hand_case((1,))
    t = up["trees"][0]
    assert up["nodes_added"] == 3 and t["left"].tolist() == [1, -1, -1] and t["right"].tolist() == [2, -1, -1]
    assert t["feature"].tolist() == [1, 0, 0] and t["default_left"].tolist() == [0, 0, 0]
    assert t["value"].tolist() == [1.0, 1.0, 1.5] and t["base_weight"].tolist() == [2.5, 2.0, 3.0]
    assert t["loss_chg"].tolist() == [2.0, 0.0, 0.0] and t["sum_hess"].tolist() == [8.0, 4.0, 4.0]
    assert t["intervals"] == [(-INF, INF)] * 3, "x1 is not constrained: the children inherit the root's interval"
    _, down = hand_case((-1,))
    t = down["trees"][0]
    assert M.same_trees(down["trees"], free["trees"])
    assert t["intervals"] == [(-INF, INF), (2.5, INF), (-INF, 2.5), (2.5, INF), (2.5, INF), (-INF, 2.5), (-INF, 2.5)]
    # the library's host code on the root's histograms: the same two decisions and intervals
    cuts, _ = hand_case(())
    bins = G.bin_rows(HAND_X, float("nan"), cuts, 2)
    q = (-(HAND_Y - F32(M.BASE)) * F32(ONE)).astype(np.int64)
    Gh, Hh = np.zeros((2, 256), np.int64), np.zeros((2, 256), np.uint64)
    for f in range(2):
        np.add.at(Gh[f], bins[f], q)
        np.add.at(Hh[f], bins[f], np.uint64(ONE))
    split = lambda cons: synth.grow_mono_node_split(Gh, Hh, cuts[0], int(q.sum()), 8 * ONE, 0.0, 0.0, 0.0, 0.0, -INF, INF, cons)
    assert split((1, 0)) == (2.0, 1, 0, 0, -8 * ONE, 4 * ONE, (-INF, INF, -INF, INF))
    assert split((-1, 0)) == (32.0, 0, 3, 0, -18 * ONE, 4 * ONE, (2.5, INF, -INF, 2.5))
    assert split((0, 0))[:6] == (32.0, 0, 3, 0, -18 * ONE, 4 * ONE)


# ---- the inputs of the GPU property test, through the restatement ----

def test_the_property_holds_on_the_restatement_and_fails_without_constraints():
    x, y, w, cuts, want = M.property_case(True)
    *_, free = M.property_case(False)
    sweeps = M.property_sweeps(x, cuts)
    assert sorted(sweeps) == [0, 2] and all(s.shape[1] > 100 for s in sweeps.values())
    broken = 0
    for f, rows in sweeps.items():
        c = M.PROPERTY["constraints"][f]
        for t in want["trees"]:
            assert M.violations(M.tree_values(t, rows), c) == 0, ("constrained", f)
        broken += sum(M.violations(M.tree_values(t, rows), c) for t in free["trees"])
    assert broken > 0, "a free tree stands against the direction: the property shows something"
    assert any(np.any(t["feature"][t["left"] >= 0] == 0) for t in want["trees"]), "the constrained trees still split on x0"
    assert not M.same_trees(want["trees"], free["trees"])
    # every node's weight lies in its interval, and a child's interval in its parent's
    for t in want["trees"]:
        for i, (lo, hi) in enumerate(t["intervals"]):
            assert F32(lo) <= t["base_weight"][i] <= F32(hi)      # (the float32 of a double in the interval)
            if t["left"][i] >= 0:
                for ch in (t["left"][i], t["right"][i]):
                    assert lo <= t["intervals"][ch][0] and t["intervals"][ch][1] <= hi


def test_all_zeros_and_the_empty_list_are_the_regularised_restatement():
    x, y, w, cuts, _, a = M.restated((0, 0, 0), "pseudohuber", 1.0, 0.5, 0.5, "rmse", 300, 282, 4)
    *_, b = RG.restated("pseudohuber", 1.0, 0.5, 0.5, "rmse", 300, 282, 4)
    assert a["nodes_added"] == b["nodes_added"] and M.same_trees(a["trees"], b["trees"])
    with pytest.raises(ValueError, match="more entries"):
        M.boost((0, 0, 0, 1), "squarederror", 1.0, 0.0, 0.0, "rmse", np.full(300, M.BASE, F32), x, float("nan"), y, w, cuts, 3)


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_mono.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_mono.hip")
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
def test_mono_kernels_resources_divisions_and_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    assert _figure(report, kernel, "VGPRs Spill") == 0 and _figure(report, kernel, "SGPRs Spill") == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body and "atomic_add" not in body and "ds_add" not in body
    assert "v_fma_mix" not in body and "v_rsq" not in body
    assert _figure(report, kernel, "VGPRs") <= 128 and _figure(report, kernel, "Occupancy [waves/SIMD]") >= 4
    # the weights divide in double by the correctly rounded sequence, never a bare reciprocal; nothing is fused but inside it
    count = lambda op: len(re.findall(op, body))
    assert count("v_div_scale_f64") >= 2 and count("v_div_fmas_f64") >= 1 and count("v_div_fixup_f64") >= 1
    assert count("v_rcp_f64") == count("v_div_fmas_f64"), "a reciprocal only inside a division"
    assert "v_rcp_f32" not in body and "v_div_scale_f32" not in body


def test_the_file_holds_its_own_kernels_and_reuses_the_rest(isa):
    text, _ = isa
    symbols = re.findall(r"^(_Z\w+):\s*; @\1$", text, re.M)
    for k in KERNELS:
        assert len([s for s in symbols if k in s]) == 1, k
    assert len(symbols) == len(KERNELS)
    csrc = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    src = open(os.path.join(csrc, "grow_mono.hip")).read()
    assert "grow_split_columns(" in src and "grow_split_nodes<" in src and "grow_deep_split_chunks(" in src
    for own in ("__shfl", "r.base_weight", "hipMemsetAsync", "hipStreamSynchronize", "for (uint32_t c0", "Ghist", "bins[", "hipFuncSetAttribute"):
        assert own not in src, own
    assert "-ffp-contract=off" in re.search(r"grow_mono_kernels\.o:.*\n\t.*", open(os.path.join(csrc, "Makefile")).read()).group(0)


# ---- the policy and a node's split under sanitizers ----

def test_the_policy_and_a_nodes_split_under_sanitizers(tmp_path):
    """tools/grow_mono_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_mono_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_mono_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert re.search(r"\d+ sums, \d+ nodes, 0 failures", r.stdout), r.stdout
