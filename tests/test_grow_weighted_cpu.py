"""Boosting with row weights, what can be checked without a GPU: the two entry points are declared, bound, exported and
placed; the header states the semantics; every refusal that needs no device, with outputs and saved bytes unchanged; the
weighted split choice and leaf solve through the host build of the shared functions on injected histograms, against the
restatement (tests/grow_weighted_support.py); the 40-pair launch plan, with the unweighted plan unchanged; the (S, W)
conversion and the comparison of two wide sums against Python integers; the new kernels cross-compile for gfx950 with
no scratch, no flat access, no float atomic and no compare-and-swap, and add with 64-bit LDS and global integer adds;
and the restatement on a case worked by hand."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_support as G
from tests import grow_weighted_support as W
from tests import helpers
from tests.test_grow_cpu import _hand_tree, kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["OHXBoosterBoostTreesWeighted", "OHXBoosterBoostTreesWeightedDevice"]
KERNELS = ["grow_hist_weighted_kernel", "grow_split_weighted_kernelILi0E", "grow_split_weighted_kernelILi1E",
           "grow_sse_weighted_kernel", "grow_walk_sse_weighted_kernel"]
SENTINEL = 12345
Q = 1 << 24


def call(b, name, dmat=None, labels=True, weights=False, eval_dmat=None, eval_labels=False, eval_weights=False,
         eval_nlabel=0, nfeat=3, rounds=2, max_depth=3, eta=0.3, lam=1.0, gamma=0.0, min_child_weight=1.0, patience=0,
         run=True, best=True, cut_ptr=True):
    """-> (rc, message); asserts that a refused call wrote no output."""
    y = np.zeros(4, dtype=np.float32)
    w = np.ones(4, dtype=np.float32)
    ptr, vals = np.arange(nfeat + 1, dtype=np.uint64), np.arange(nfeat, dtype=np.float32)
    train = np.full(rounds + 1 if rounds > 0 else 1, -7.0)
    held = train.copy()
    r, k, n = C.c_int32(SENTINEL), C.c_int32(SENTINEL), C.c_uint64(SENTINEL)
    args = [b.handle, dmat, y.ctypes.data if labels else None, w.ctypes.data if weights else None, 4, eval_dmat,
            y.ctypes.data if eval_labels else None, w.ctypes.data if eval_weights else None, eval_nlabel,
            ptr.ctypes.data if cut_ptr else None, vals.ctypes.data, rounds, max_depth, eta, lam, gamma, min_child_weight,
            patience, train.ctypes.data, held.ctypes.data, C.byref(r) if run else None, C.byref(k) if best else None,
            C.byref(n)]
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
        assert header.index("int OHXBoosterBoostTreesEvalDevice(") < header.index("int " + name + "(") < header.index("int OHXQuantileCuts(")
        assert f90.index('name="OHXBoosterBoostTreesEvalDevice"') < f90.index(f'name="{name}"') < f90.index('name="OHXQuantileCuts"')
    for method in ("boost_trees_weighted", "boost_trees_weighted_device"):
        assert hasattr(capi.Booster, method)
    for f in ("grow_plan_weighted", "boost_weighted_rmse", "boost_weighted_compare", "grow_node_split_weighted"):
        assert hasattr(synth, f)


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    header = re.sub(r"\s*\n \*\s*", " ", header)          # comment lines joined
    for phrase in ("NULL means every weight is 1.0f", "w is finite with 0 <= w < 256", "hq = (uint64) rint(w * 2^24)",
                   "looks at g before the weight", "gw = g * w is one float32 multiply, not fused",
                   "q = (int64) rint(gw * 2^24)", "the uint64 sum of hq", "a sum of hq is < 2^63",
                   "no float atomics, no compare-and-swap", "Hd = (double)H * 2^-24",
                   "gain(G, H) = (Gd * Gd) / (Hd + (double)lambda)", "base_weight = (float)( -Gd / (Hd + (double)lambda) )",
                   "sum_hess = (float)Hd", "HL > 0 and HR > 0 as integers", "HLd >= (double)min_child_weight",
                   "Hd < 2 * min_child_weight", "S_t = sum_r hq_r * e_r^2 is an exact integer < 2^127",
                   "sqrt( ((double)S_t * 2^-72) / ((double)W * 2^-24) )", "unsigned __int128, rounded to nearest even",
                   "P2 += (hq * a) >> 32", "P1 += ((hq * a) & m) + ((hq * b) >> 32)", "P0 += (hq * b) & m",
                   "none of the accumulators can overflow", "equal those of OHXBoosterBoostTreesEval",
                   "A weight-0 row influences no tree and no sum", "equals that many copies of the row",
                   "\"eval weight\"", "whose W is 0", "eval_weights given without a held-out matrix",
                   "eval_weights must then be NULL", "Not capturable"):
        assert phrase in header, phrase


# ---- refusals that need no device ----

@pytest.mark.parametrize("name", SYMBOLS)
def test_no_model_is_refused(name):
    rc, msg = call(capi.Booster(), name)
    assert rc == -1 and "holds no model" in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
def test_bad_arguments_are_refused_before_a_matrix_is_looked_at(name):
    js, _ = S.make_booster(11, 3)
    import json
    F = int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    # what the Eval call refuses, under this call's name
    rc, msg = call(b, name, nfeat=F, labels=False)
    assert rc == -1 and name in msg and "labels is NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, cut_ptr=False)
    assert rc == -1 and "the cuts are NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, rounds=0)
    assert rc == -1 and "rounds must be >= 1" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=9)
    assert rc == -1 and "max_depth must be in 1..8" in msg, msg
    rc, msg = call(b, name, nfeat=F, lam=-1.0)
    assert rc == -1 and "lambda must be finite and >= 0" in msg, msg
    for p in (-1, -100):
        rc, msg = call(b, name, nfeat=F, patience=p)
        assert rc == -1 and "patience must be >= 0" in msg, msg
    for kw in ({"run": False}, {"best": False}):
        rc, msg = call(b, name, nfeat=F, **kw)
        assert rc == -1 and "rounds_run or best_round is NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, patience=2)
    assert rc == -1 and "needs a held-out matrix" in msg, msg
    rc, msg = call(b, name, nfeat=F, eval_labels=True, eval_nlabel=4)
    assert rc == -1 and "eval labels are given without a held-out matrix" in msg, msg
    # its own
    for bad in (float("nan"), float("inf"), float("-inf"), -1.0, -1e-30):
        rc, msg = call(b, name, nfeat=F, min_child_weight=bad)
        assert rc == -1 and name in msg and "min_child_weight must be finite and >= 0" in msg, msg
    rc, msg = call(b, name, nfeat=F, eval_weights=True)
    assert rc == -1 and name in msg and "eval weights are given without a held-out matrix" in msg, msg
    rc, msg = call(b, name, nfeat=F, weights=True, eval_weights=True)
    assert rc == -1 and "eval weights are given without a held-out matrix" in msg, msg
    # a held-out handle without labels (the handle is not looked at yet), with weights
    rc, msg = call(b, name, nfeat=F, eval_dmat=C.c_void_p(0x1000), eval_nlabel=4, eval_weights=True)
    assert rc == -1 and "eval labels is NULL" in msg, msg
    # an earlier refusal wins over a later one
    rc, msg = call(b, name, nfeat=F, rounds=0, min_child_weight=-1.0)
    assert rc == -1 and "rounds must be >= 1" in msg, msg
    rc, msg = call(b, name, nfeat=F, min_child_weight=-1.0, patience=-1)
    assert rc == -1 and "min_child_weight" in msg, msg
    # every argument sound (min_child_weight 0 and weights given are both legal): the NULL matrix is what is left
    for kw in ({}, {"min_child_weight": 0.0}, {"weights": True, "rounds": 7, "max_depth": 8, "min_child_weight": 1e30}):
        rc, msg = call(b, name, nfeat=F, **kw)
        assert rc == -1 and "DMatrix handle is invalid" in msg, msg
    assert saved(b) == before, "a refusal changed the forest"


# ---- the weighted split choice on injected histograms ----

def _split_case(Gh, Hh, ncuts, lam=1.0, gamma=0.0, mcw=0.0):
    Gh = np.asarray(Gh, dtype=np.int64)
    Hh = np.asarray(Hh, dtype=np.uint64)
    ptr = np.concatenate([[0], np.cumsum(ncuts)]).astype(np.uint64)
    Gp, Hp = int(Gh[0].sum()), sum(int(h) for h in Hh[0])
    for f in range(len(Gh)):
        assert int(Gh[f].sum()) == Gp and sum(int(h) for h in Hh[f]) == Hp, "every row is in one bin of every feature"
    got = synth.grow_node_split_weighted(Gh, Hh, ptr, Gp, Hp, lam, gamma, mcw)
    want = W.best_split(Gh, Hh, ncuts, Gp, Hp, lam, mcw)
    assert not math.isnan(got["loss_chg"])
    if want is None:
        assert not got["valid"] and not got["splits"]
        return got
    loss, f, j, dl, GL, HL = want
    assert got["valid"] and (got["feature"], got["j"], got["default_left"]) == (f, j, dl), (got, want)
    assert np.float64(got["loss_chg"]).view(np.uint64) == np.float64(loss).view(np.uint64)
    assert (got["GL"], got["HL"]) == (GL, HL)
    assert got["splits"] == bool(loss > float(np.float32(gamma)))
    return got


def _hist(nfeat):
    return np.zeros((nfeat, 256), np.int64), np.zeros((nfeat, 256), np.uint64)


def test_split_with_fractional_hessians_by_hand():
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = -5 * Q, 7 * Q // 2          # H = 3.5
    Gh[0, 1], Hh[0, 1] = -16 * Q, 4 * Q
    got = _split_case(Gh, Hh, [1], lam=0.0)
    assert got["valid"] and got["splits"] and got["HL"] == 7 * Q // 2
    assert got["loss_chg"] == (25.0 / 3.5 + 64.0) - 441.0 / 7.5


def test_split_an_empty_child_with_lambda_zero_is_invalid_and_no_nan():
    # the only cut leaves nothing on the left: HL == 0, lambda == 0 would divide 0 by 0
    Gh, Hh = _hist(1)
    Gh[0, 1], Hh[0, 1] = 3 * Q, 2 * Q
    got = _split_case(Gh, Hh, [1], lam=0.0)
    assert not got["valid"] and got["loss_chg"] == 0.0
    # gradient without hessian on the left (weights below the fixed point's resolution): still invalid
    Gh[0, 0] = 17
    got = _split_case(Gh, Hh, [1], lam=0.0)
    assert not got["valid"]
    # with a second cut that is valid, the empty one is passed over
    Gh, Hh = _hist(1)
    Gh[0, 1], Hh[0, 1] = -3 * Q, 2 * Q
    Gh[0, 2], Hh[0, 2] = 3 * Q, 2 * Q
    got = _split_case(Gh, Hh, [2], lam=0.0)
    assert got["valid"] and got["j"] == 1
    # everything in the missing bin: dl = 1 empties the right child, dl = 0 the left
    Gh, Hh = _hist(1)
    Gh[0, 255], Hh[0, 255] = 3 * Q, 2 * Q
    assert not _split_case(Gh, Hh, [3], lam=0.0)["valid"]


def test_split_exact_ties():
    Gh, Hh = _hist(3)
    for f in (1, 2):                              # two identical features behind one that cannot split
        Gh[f, 0], Hh[f, 0] = -4 * Q, Q // 2
        Gh[f, 1], Hh[f, 1] = 4 * Q, Q // 2
    Gh[0, 0], Hh[0, 0] = 0, Q
    assert _split_case(Gh, Hh, [1, 1, 1])["feature"] == 1
    # bins (a, 0, b): cuts 0 and 1 make the same children; no missing rows: both defaults tie
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = -4 * Q, 3 * Q
    Gh[0, 2], Hh[0, 2] = 4 * Q, 3 * Q
    got = _split_case(Gh, Hh, [2])
    assert (got["j"], got["default_left"]) == (0, 0)


def test_split_min_child_weight():
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = -50 * Q, Q // 2           # the best cut isolates weight 0.5
    Gh[0, 1], Hh[0, 1] = 2 * Q, 3 * Q
    Gh[0, 2], Hh[0, 2] = 3 * Q, 4 * Q
    assert _split_case(Gh, Hh, [2], mcw=0.0)["j"] == 0
    assert _split_case(Gh, Hh, [2], mcw=0.5)["j"] == 0
    assert _split_case(Gh, Hh, [2], mcw=float(np.nextafter(np.float32(0.5), np.float32(1))))["j"] == 1
    assert _split_case(Gh, Hh, [2], mcw=3.5)["j"] == 1
    assert not _split_case(Gh, Hh, [2], mcw=3.75)["valid"], "Hd = 7.5 < 2 * 3.75 is false, but no child pair has 3.75 each"
    assert not _split_case(Gh, Hh, [2], mcw=4.0)["valid"], "Hd < 2 * min_child_weight: a leaf without evaluation"


def test_split_random_histograms_against_the_restatement():
    rng = np.random.default_rng(1)
    for case in range(40):
        nf = int(rng.integers(1, 6))
        ncuts = rng.integers(0, 255, nf)
        Gh, Hh = _hist(nf)
        n = int(rng.integers(2, 400))
        w = rng.choice([0.0, 0.5, 1.0, 2.0, 100.0], n).astype(np.float32) if case % 2 else (rng.random(n) * 4).astype(np.float32)
        g = rng.uniform(-2, 2, n).astype(np.float32)
        hq = W.hess_fixed(w)
        q = W.grad_fixed(g, w)
        for f in range(nf):
            b = rng.integers(0, ncuts[f] + 1, n)
            b[rng.random(n) < 0.2] = 255
            np.add.at(Gh[f], b, q)
            np.add.at(Hh[f], b, hq)
        _split_case(Gh, Hh, ncuts, lam=float(rng.choice([0.0, 1.0])), mcw=float(rng.choice([0.0, 0.5, 3.0])))
    # sums past 2^53: the conversion of H rounds
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = (1 << 53) + 1, (1 << 61) + 1
    Gh[0, 1], Hh[0, 1] = -(1 << 53) - 3, (1 << 61) + 3
    _split_case(Gh, Hh, [1], lam=0.0)


def test_the_two_hessian_policies_choose_the_same_split_of_unit_weights():
    """One scan and one node split serve both hessian policies (grow.hpp): the count policy on (G, H) and the
    fixed-point policy on (G, H << 24) with min_child_weight = (float)min_child_rows give the same key, loss_chg, GL
    and HL - (double)H and (double)(H << 24) * 2^-24 are the same double, and HL < min_child_rows covers HL == 0."""
    rng = np.random.default_rng(22)
    cases = 0
    for case in range(48):
        nf = (1, 3)[case % 2]
        ncuts = rng.integers(1, 255, nf)
        n = int(rng.integers(2, 300))
        q = W.grad_fixed(rng.uniform(-2, 2, n).astype(np.float32), np.ones(n, np.float32))
        Gh, Hh = _hist(nf)
        for f in range(nf):
            b = rng.integers(0, ncuts[f] + 1, n)
            b[rng.random(n) < 0.2] = 255
            np.add.at(Gh[f], b, q)
            np.add.at(Hh[f], b, np.uint64(1))
        ptr = np.concatenate([[0], np.cumsum(ncuts)]).astype(np.uint64)
        Gp = int(Gh[0].sum())
        for mcr in (1, 2, n // 2 + 1):
            for lam in (0.0, 1.0):
                count = synth.grow_node_split(Gh, Hh, ptr, Gp, n, lam, 0.0, mcr)
                fixed = synth.grow_node_split_weighted(Gh, Hh << np.uint64(24), ptr, Gp, n << 24, lam, 0.0, float(mcr))
                for k in ("valid", "feature", "j", "default_left", "splits", "GL"):
                    assert count[k] == fixed[k], (case, mcr, lam, k, count, fixed)
                assert np.float64(count["loss_chg"]).view(np.uint64) == np.float64(fixed["loss_chg"]).view(np.uint64)
                assert count["HL"] == fixed["HL"] >> 24 and fixed["HL"] & ((1 << 24) - 1) == 0
                if mcr == n // 2 + 1:
                    assert not count["valid"], "no two children hold more than half the rows each"
                cases += count["valid"]
    assert cases > 100, "most cases have a split to compare"


def test_the_leaf_solve():
    for Gs, H, eta, lam in ((-5 * Q, 7 * Q // 2, 1.0, 0.0), (3 * Q + 1, Q // 3, 0.3, 1.0), (0, Q, 0.5, 0.0),
                            (-(1 << 60) - 1, (1 << 62) + 5, 0.1, 1e-3), (17, 1, 1.0, 0.0)):
        got = synth.grow_solve_leaf_weighted(Gs, H, eta, lam)
        want = W.solve(Gs, H, eta, lam)
        assert [helpers.bits(np.float32(v)).item() for v in got] == [helpers.bits(np.float32(v)).item() for v in want], (Gs, H)
    leaf, w, sh = synth.grow_solve_leaf_weighted(-5 * Q, 7 * Q // 2, 1.0, 0.0)
    assert w == np.float32(5.0 / 3.5) and sh == np.float32(3.5)


# ---- the launch plan ----

@pytest.mark.parametrize("nrow", [1, 63, 4097, 1 << 20, 55987200, 1 << 31])
@pytest.mark.parametrize("nfeat", [1, 3, 27, 40, 41, 128])
def test_the_weighted_plan(nrow, nfeat):
    cus = 256
    p = synth.grow_plan_weighted(nrow, nfeat, nfeat * 254, 8, cus)
    u = synth.grow_plan(nrow, nfeat, nfeat * 254, 8, cus)
    assert p["max_pairs"] == 40 and p["pair_bytes"] == 256 * 16 and p["hist_block_rows"] == 1024
    for k in ("row_blocks", "block_rows", "bin_lds_bytes", "bins_bytes", "hist_bytes"):
        assert p[k] == u[k], k
    assert len(p["levels"]) == 8
    for d, l in enumerate(p["levels"]):
        assert l["slots"] == 1 << d
        assert l["node_group"] * l["feat_group"] <= 40
        assert l["lds_bytes"] == l["node_group"] * l["feat_group"] * 256 * 16 <= 160 * 1024
        for total, size, groups in ((l["slots"], l["node_group"], l["node_groups"]), (nfeat, l["feat_group"], l["feat_groups"])):
            assert size >= 1 and groups * size >= total and (groups - 1) * size < total
        assert l["hist_blocks"] >= 1 and (l["hist_blocks"] - 1) * 1024 < nrow
        assert l["hist_blocks"] * l["node_groups"] * l["feat_groups"] <= max(cus * 2, l["node_groups"] * l["feat_groups"])


def test_the_unweighted_plan_is_unchanged():
    """The figures docs/18_boost_trees.md quotes for the benchmark shape, and the 53-pair rule at every level."""
    p = synth.grow_plan(55987200, 27, 6639, 6, 256)
    assert p["max_pairs"] == 53 and p["pair_bytes"] == 256 * 12
    assert [(l["node_group"], l["feat_group"], l["node_groups"], l["feat_groups"]) for l in p["levels"]] == [
        (1, 27, 1, 1), (2, 14, 1, 2), (4, 9, 1, 3), (8, 6, 1, 5), (16, 3, 1, 9), (32, 1, 1, 27)]
    w = synth.grow_plan_weighted(55987200, 27, 6639, 6, 256)
    assert [(l["node_group"], l["feat_group"], l["node_groups"], l["feat_groups"]) for l in w["levels"]] == [
        (1, 27, 1, 1), (2, 14, 1, 2), (4, 9, 1, 3), (8, 5, 1, 6), (16, 2, 1, 14), (32, 1, 1, 27)]
    for nfeat in (1, 53, 54, 128):
        for l in synth.grow_plan(4097, nfeat, 0, 8, 256)["levels"]:
            ng = min(l["slots"], 53)
            fg = max(1, min(nfeat, 53 // ng))
            groups = -(-nfeat // fg)
            assert (l["node_group"], l["feat_groups"], l["feat_group"]) == (ng, groups, -(-nfeat // groups))
            assert l["lds_bytes"] == l["node_group"] * l["feat_group"] * 256 * 12


# ---- the (S, W) conversion and the comparison ----

def _parts(Sx, spread=0):
    """S as (p2, p1, p0); spread 1 / 2: p0 / p1 left un-normalised where the part above has something to lend."""
    p2, p1, p0 = Sx >> 64, (Sx >> 32) & 0xFFFFFFFF, Sx & 0xFFFFFFFF
    if spread == 1 and p1 > 0:
        p1, p0 = p1 - 1, p0 + (1 << 32)
    if spread == 2 and p2 > 0:
        p2, p1 = p2 - 1, p1 + (1 << 32)
    return p2, p1, p0


def test_weighted_rmse_conversion_against_python_integers():
    cases = [(0, 7 * Q), (1, Q), (1, 1), ((1 << 64) - 1, Q), ((1 << 64) - 1, 4097 * Q + 5), (1 << 100, 1 << 55),
             ((1 << 100) + 12345678901, (1 << 55) - 1), ((1 << 100) - 1, 3), (1 << 126, 1 << 62), ((1 << 126) + (1 << 73) + 1, (1 << 63) - 1),
             ((1 << 127) - 1, (1 << 63) - 1),
             # 54 and more bits: rounding to 53 bits both ways, and the ties to even
             ((1 << 53) + 1, 3 * Q), ((1 << 53) + 3, 3 * Q), ((1 << 80) + (1 << 27), 5), ((1 << 80) + (1 << 27) + 1, 5),
             ((1 << 80) + (3 << 27), 5), ((1 << 80) + (3 << 27) - 1, 5), ((1 << 120) + (1 << 67), (1 << 53) + 1),
             ((1 << 120) + (3 << 67), (1 << 53) + 3), (5 << 72, (1 << 60) + (1 << 7)), (5 << 72, (1 << 60) + (3 << 7))]
    rng = np.random.default_rng(3)
    for _ in range(200):
        cases.append((int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 65)) | int(rng.integers(0, 1 << 20)),
                      int(rng.integers(1, 1 << 62))))
    down = up = wdown = wup = 0
    for Sx, Wx in cases:
        assert Sx < 1 << 127 and 0 < Wx < 1 << 63
        want = W.rmse(Sx, Wx)
        down += int(float(Sx)) < Sx
        up += int(float(Sx)) > Sx
        wdown += int(float(Wx)) < Wx
        wup += int(float(Wx)) > Wx
        for spread in (0, 1, 2):
            got = synth.boost_weighted_rmse(*_parts(Sx, spread), Wx)
            assert got == want, (Sx, Wx, spread, got, want)
    assert down > 10 and up > 10 and wdown > 10 and wup > 10, "cases rounded both ways"
    assert synth.boost_weighted_rmse(0, 0, 0, 5) == 0.0
    assert synth.boost_weighted_rmse(0, 0, 1, 1) == 2.0 ** -24
    assert synth.boost_weighted_rmse(1, 0, 0, Q) == 2.0 ** -4 and synth.boost_weighted_rmse(1 << 8, 0, 0, Q) == 1.0


def test_the_carries_between_the_three_accumulators():
    """Each accumulator as large as 2^31 rows can make it: p2, p0 < 2^63, p1 <= 2^64 - 2^32."""
    M = (1 << 32) - 1
    for p2, p1, p0 in (((1 << 63) - (1 << 33), (1 << 64) - (1 << 32), (1 << 63) - 1), (0, (1 << 64) - (1 << 32), 0), (0, 0, (1 << 63) - 1),
                       (7, M << 32, M << 31), (0, 1, 1 << 32), (1, 0, 0), (0, 1 << 32, 0), (0, 0, 1 << 62)):
        Sx = (p2 << 64) + (p1 << 32) + p0
        assert Sx < 1 << 127
        assert synth.boost_weighted_rmse(p2, p1, p0, 3 * Q) == W.rmse(Sx, 3 * Q), (p2, p1, p0)
    # the same integer written three ways compares equal; one more is more
    a, b, c = (1, 0, 0), (0, 1 << 32, 0), (0, (1 << 32) - 1, 1 << 32)
    assert synth.boost_weighted_compare(a, b) == 0 and synth.boost_weighted_compare(b, c) == 0
    assert synth.boost_weighted_compare((0, (1 << 32) - 1, (1 << 32) + 1), a) == 1
    assert synth.boost_weighted_compare(a, (0, (1 << 32) - 1, (1 << 32) + 1)) == -1
    assert synth.boost_weighted_compare((5, 7, 9), (5, 7, 8)) == 1 and synth.boost_weighted_compare((5, 6, M), (5, 7, 0)) == -1
    assert synth.boost_weighted_compare((4, (1 << 64) - (1 << 32), 0), (5, 0, 0)) == 1
    # the stop rule over wide sums is the rule of the Eval call
    v = [(1 << 100) + d for d in (10, 5, 6, 7, 4, 8, 9, 9, 1)]
    assert synth.boost_weighted_stop([_parts(s) for s in v], 3) == (7, 4)
    assert synth.boost_weighted_stop([_parts(s, 2) for s in v], 1) == (2, 1)
    assert synth.boost_weighted_stop([_parts(s) for s in [v[0]] * 4], 1) == (1, 0), "a tie is not an improvement"


def test_the_device_parts_add_up_to_the_exact_sum():
    """The header's P2, P1, P0 against S as a Python int, at the edges of every factor."""
    edge = np.float32(256.0 - 2.0 ** -16)
    g = np.array([edge, -edge, 2.0 ** -24, 0.0, 1.0, -0.3, 255.0], np.float32)
    w = np.array([edge, 1.0, edge, 3.0, 2.0 ** -24, 0.7, 0.0], np.float32)
    hq = W.hess_fixed(w)
    assert int(hq[0]) == (1 << 32) - 256 and int(hq[4]) == 1 and int(hq[6]) == 0
    P2, P1, P0 = W.parts(g, hq)
    Sx, Wx = W.weighted_sum(g, hq)
    assert (P2 << 64) + (P1 << 32) + P0 == Sx and Sx > 1 << 95
    assert synth.boost_weighted_rmse(P2, P1, P0, Wx) == W.rmse(Sx, Wx)
    # 2^31 such rows overflow nothing
    worst = ((1 << 32) - 256) ** 2
    a, b, h = worst >> 32, worst & 0xFFFFFFFF, (1 << 32) - 1
    assert ((h * a) >> 32) << 31 < 1 << 63 and (((h * a) & 0xFFFFFFFF) + ((h * b) >> 32)) << 31 < 1 << 64
    assert ((1 << 33) - 2) << 31 == (1 << 64) - (1 << 32)


def test_unit_weights_give_the_rmse_of_the_eval_call():
    rng = np.random.default_rng(4)
    for n in (1, 3, 4097, (1 << 31) - 1, 1 << 31):
        for _ in range(20):
            Sq = int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 32))         # sum q^2 < 2^95
            hi, lo = Sq >> 32, Sq & 0xFFFFFFFF
            assert synth.boost_weighted_rmse(*_parts(Sq << 24), n << 24) == synth.boost_eval_rmse(hi, lo, n), (Sq, n)


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_weighted.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_weighted.hip")
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
def test_weighted_kernels_resources_and_atomics(isa, kernel):
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
    elif "walk" in kernel:
        assert adds == 3 and "ds_add" not in body, "p2, p1, p0"
    elif "sse" in kernel:
        assert adds == 4 and "ds_add" not in body, "p2, p1, p0 and W"
    else:
        assert "atomic_add" not in body and "ds_add" not in body
    if "ILi0E" in kernel:
        assert "v_div_scale_f64" in body, "the gain divides in double"
    assert _figure(report, kernel, "ScratchSize [bytes/lane]") == 0
    lds = {"grow_hist_weighted_kernel": 0, "grow_split_weighted_kernelILi0E": 0, "grow_split_weighted_kernelILi1E": 256 * 4,
           "grow_sse_weighted_kernel": 4 * 4 * 8, "grow_walk_sse_weighted_kernel": 512 * 16 + 4 * 4 * 8}[kernel]
    assert _figure(report, kernel, "LDS Size [bytes/block]") == lds, "static LDS (the histogram's is dynamic)"
    # registers: the streaming kernels keep 8 waves a SIMD (at most 64 VGPRs); the split kernels need at least 4
    vgprs, occupancy = _figure(report, kernel, "VGPRs"), _figure(report, kernel, "Occupancy [waves/SIMD]")
    if "split" in kernel:
        assert vgprs <= 128 and occupancy >= 4, (vgprs, occupancy)
    else:
        assert vgprs <= 64 and occupancy == 8, (vgprs, occupancy)


def test_the_earlier_kernel_files_hold_no_weighted_kernel():
    for name in ("grow.hip", "grow_eval.hip"):
        src = open(os.path.join(helpers.ROOT, "quickchem_amd", "csrc", name)).read()
        assert "weighted" not in src.replace("grow_weighted.hip", ""), name
    src = open(os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_weighted.hip")).read()
    assert sorted(set(re.findall(r"void (grow_\w+_kernel)\(", src))) == sorted(
        ["grow_hist_weighted_kernel", "grow_split_weighted_kernel", "grow_sse_weighted_kernel", "grow_walk_sse_weighted_kernel"])
    # the held-out rows' walk is one text: the node, the staging and the walk are the shared header's, and both metric
    # files call them and step through no tree[p] of their own
    shared = open(os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_device.hpp")).read()
    assert "weighted" not in shared and "sampled" not in shared, "the shared text takes neither file's word"
    for what in ("struct EvalNode", "grow_stage_tree(const", "grow_walk_row(const"):
        assert shared.count(what) == 1, what
    assert "tree[p]" in shared
    for name in ("grow_eval.hip", "grow_weighted.hip"):
        src = open(os.path.join(helpers.ROOT, "quickchem_amd", "csrc", name)).read()
        assert '#include "grow_device.hpp"' in src, name
        assert "grow_stage_tree(" in src and "grow_walk_row(" in src, name
        assert "tree[p]" not in src and "struct EvalNode" not in src, name


# ---- the host functions under sanitizers ----

def test_the_host_functions_under_sanitizers(tmp_path):
    """tools/grow_weighted_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only): the plan,
    the (S, W) conversion and comparison, and the weighted split on histograms with the largest sums 2^31 rows make."""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    exe = tmp_path / "grow_weighted_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", src,
                            os.path.join(helpers.ROOT, "tools", "grow_weighted_host_check.cpp"), os.path.join(src, "grow.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)    # (grow.cpp's tree assembly, the one function
    # that needs forest_io.cpp, is not called and its section is dropped)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe), "300", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


# ---- the restatement itself ----

def test_the_restatement_on_a_case_worked_by_hand():
    """The 8 rows of test_grow_cpu's hand case with weights 1, 2, 0, 0.5, 1, 1, 0, 2; base 0, eta 1, lambda 0, depth 2.
    g * w = 0, -4, 0, -1, -4, -4, 0, -8.  Root: G = -21, H = 7.5, gain 58.8.  f0: rows 0-3 left, G = -5, H = 3.5 and
    right G = -16, H = 4: 25/3.5 + 64 - 58.8.  f1: -4 | -17 with H 2 | 5.5: 8 + 289/5.5 - 58.8, smaller.  Node 1 (G = -5,
    H = 3.5): f1: rows 0, 2 left (G = 0, H = 1), rows 1, 3 right (G = -5, H = 2.5): 0 + 10 - 25/3.5 > 0: splits.  Node 2
    (G = -16, H = 4): f1: -4 | -12 with H 1 | 3: 16 + 48 - 64 = 0, not above gamma: a leaf of 4.  Leaves: -0.0, 5/2.5 = 2.
    Every row is fitted: S_1 = 0; S_0 = sum w y^2 * 2^72 = (8 + 2 + 16 + 16 + 32) * 2^72, W = 7.5 * 2^24."""
    x, y, cuts = _hand_tree()
    w = np.array([1, 2, 0, 0.5, 1, 1, 0, 2], np.float32)
    z = np.zeros(8, np.float32)
    out = W.boost_weighted(z, x, float("nan"), y, w, cuts, 2, rounds=1, max_depth=2, eta=1.0, lam=0.0, min_child_weight=0.0)
    t = out["trees"][0]
    lb = -(1 << 31)
    assert t["left"].tolist() == [1, 3, -1, -1, -1] and t["right"].tolist() == [2, 4, -1, -1, -1]
    assert t["parent"].tolist() == [-1, 0 + lb, 0, 1 + lb, 1]
    assert t["feature"].tolist() == [0, 1, 0, 0, 0] and t["default_left"].tolist() == [0, 0, 0, 0, 0]
    assert t["value"].tolist() == [2.0, 2.0, 4.0, 0.0, 2.0] and np.signbit(t["value"][3])
    assert t["loss_chg"].tolist() == [np.float32((25.0 / 3.5 + 64.0) - 441.0 / 7.5), np.float32((0.0 + 10.0) - 25.0 / 3.5), 0.0, 0.0, 0.0]
    assert t["sum_hess"].tolist() == [7.5, 3.5, 4.0, 1.0, 2.5]
    assert t["base_weight"].tolist() == [np.float32(21.0 / 7.5), np.float32(5.0 / 3.5), 4.0, 0.0, 2.0]
    assert out["train_sums"] == [74 << 72, 0] and out["train_W"] == 15 * Q // 2
    assert out["train_rmse"] == [math.sqrt(74.0 / 7.5), 0.0] and out["pred"].tolist() == y.tolist()
    assert out["nodes_added"] == 5 and (out["rounds_run"], out["best_round"]) == (1, 1)
    # the library's host functions on the same sums
    assert synth.boost_weighted_rmse(74 << 8, 0, 0, 15 * Q // 2) == out["train_rmse"][0]
    # min_child_weight 2: node 1 (H = 3.5 < 4) stays a leaf of 5/3.5; the root still splits (3.5 and 4 both >= 2)
    out = W.boost_weighted(z, x, float("nan"), y, w, cuts, 2, rounds=1, max_depth=2, eta=1.0, lam=0.0, min_child_weight=2.0)
    assert out["trees"][0]["left"].tolist() == [1, -1, -1] and out["trees"][0]["value"][1] == np.float32(5.0 / 3.5)
    # held out on itself with the same weights: the same sums; with patience 1 a second, empty round ties and stops
    out = W.boost_weighted(z, x, float("nan"), y, w, cuts, 2, eval_set=(x, float("nan"), y, w), eval_pred=z, rounds=5,
                           patience=1, max_depth=2, eta=1.0, lam=0.0, min_child_weight=0.0)
    assert out["eval_sums"] == [74 << 72, 0, 0] and (out["rounds_run"], out["best_round"]) == (2, 1)
    # unit weights: the Eval restatement's trees and sums
    from tests import grow_eval_support as E
    a = W.boost_weighted(z, x, float("nan"), y, None, cuts, 2, rounds=2, max_depth=2, eta=1.0, lam=0.0, min_child_weight=1.0)
    e = E.boost_eval(z, x, float("nan"), y, cuts, 2, rounds=2, max_depth=2, eta=1.0, lam=0.0)
    assert a["train_rmse"] == e["train_rmse"] and [s >> 24 for s in a["train_sums"]] == e["train_sums"]
    for ta, te in zip(a["trees"], e["trees"]):
        assert all(np.array_equal(ta[k], te[k]) for k in G.ARRAYS)
    # refusals, in the header's order: the label before the weight
    bad = w.copy()
    bad[2] = np.nan
    with pytest.raises(ValueError, match="^weight"):
        W.boost_weighted(z, x, float("nan"), y, bad, cuts, 2)
    yb = y.copy()
    yb[2] = np.nan
    with pytest.raises(ValueError, match="^label"):
        W.boost_weighted(z, x, float("nan"), yb, bad, cuts, 2)
    with pytest.raises(ValueError, match="^label"):                  # |g| = 4 < 256, |g * w| = 800
        W.boost_weighted(z, x, float("nan"), y, np.full(8, 200.0, np.float32), cuts, 2)
    with pytest.raises(ValueError, match="sum to 0"):
        W.boost_weighted(z, x, float("nan"), y, np.zeros(8, np.float32), cuts, 2)
