"""Boosting new trees, what can be checked without a GPU: the three entry points are declared, bound and exported; every
refusal that needs no device, with its message and the forest's saved bytes unchanged; OHXQuantileCuts against the
restatement; the split choice on injected histograms through the host build of the shared function; the tree assembly
through all three file formats; the launch plan; the kernels cross-compile for gfx950 with no scratch, no flat memory
instructions, no float atomic and no compare-and-swap; and the numpy restatement (tests/grow_support.py) on a case worked
by hand."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import categorical_support as CS
from tests import grow_support as G
from tests import helpers
from tests import output_groups_support as OG
from tests import visits_support as V

HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["OHXBoosterBoostTrees", "OHXBoosterBoostTreesDevice"]
KERNELS = ["grow_bin_kernel", "grow_hist_kernel", "grow_split_kernelILi0E", "grow_split_kernelILi1E",
           "grow_partition_kernel", "grow_leaf_kernel"]
Q = 1 << 24


def call(b, name, dmat=None, labels=True, cut_ptr=True, cut_values=True, nfeat=3, rounds=1, max_depth=3, eta=0.3,
         lam=1.0, gamma=0.0, min_child_rows=1, cuts=None):
    """-> (rc, message)."""
    y = np.zeros(4, dtype=np.float32)
    ptr, vals = cuts if cuts is not None else (np.arange(nfeat + 1, dtype=np.uint64), np.arange(nfeat, dtype=np.float32))
    ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    n = C.c_uint64(12345)
    args = [b.handle, dmat, y.ctypes.data if labels else None, 4, ptr.ctypes.data if cut_ptr else None,
            vals.ctypes.data if cut_values else None, rounds, max_depth, eta, lam, gamma, min_child_rows, C.byref(n)]
    if name.endswith("Device"):
        args.append(None)
    rc = getattr(b.lib, name)(*args)
    assert rc == 0 or n.value == 12345, "a refused call wrote nodes_added"
    return rc, b.lib.XGBGetLastError().decode()


def saved(b, formats=("json", "ubj", "bin")):
    with tempfile.TemporaryDirectory() as d:
        out = []
        for ext in formats:
            path = os.path.join(d, "m." + ext)
            b.save_model(path)
            out.append(open(path, "rb").read())
    return out


def test_entry_points_declared_bound_and_exported():
    lib = C.CDLL(helpers.PRODUCT_SO)
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    f90 = open(os.path.join(helpers.ROOT, "quickchem_amd", "fortran", "ohx_bindings.F90")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    for name in SYMBOLS + ["OHXQuantileCuts"]:
        assert name in capi.ABI_SYMBOLS
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert re.search(r" T " + name + r"$", nm, re.M), name
        assert f'bind(C, name="{name}")' in f90, name
        # after the refit block
        assert header.index("int OHXBoosterRefitLeavesDevice(") < header.index("int " + name + "(")
    for method in ("boost_trees", "boost_trees_device"):
        assert hasattr(capi.Booster, method)
    assert hasattr(capi, "quantile_cuts")


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    header = re.sub(r"\s*\n \*\s*", " ", header)          # comment lines joined
    for phrase in ("b = #{j : c_j <= x}", "the missing bin, 255", "x < c_j exactly when b <= j",
                   "s[floor(j * n / max_bins)]", "left = n, right = n + 1", "Integer adds only",
                   "gain(G, H) = (Gd * Gd) / ((double)H + (double)lambda)", "loss_chg = (gain(L) + gain(R)) - gain(P)",
                   "no fused multiply-add", "lexicographically smallest (f, j, dl)", "best > (double)gamma",
                   "Hp < 2 * min_child_rows", "All or nothing", "WITH its counters", "Both forms wait once",
                   "HOST pointers in both forms", "\"ohx_device\" move", "is NOT claimed"):
        assert phrase in header, phrase


# ---- refusals that need no device ----

@pytest.mark.parametrize("name", SYMBOLS)
def test_no_model_is_refused(name):
    rc, msg = call(capi.Booster(), name)
    assert rc == -1 and "holds no model" in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
def test_a_categorical_booster_is_refused_at_the_top(name):
    js, _, _ = CS.make_booster(5, 3)
    b = capi.Booster(model_buffer=js)
    before = saved(b, ("json", "ubj"))        # (the legacy format holds no categorical split)
    rc, msg = call(b, name)
    assert rc == -1 and "categorical" in msg and name in msg, msg
    assert saved(b, ("json", "ubj")) == before


@pytest.mark.parametrize("name", SYMBOLS)
def test_several_output_groups_are_refused_at_the_top(name):
    js, _, _ = OG.make_multi(8, 6, 3, "round_robin")
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    rc, msg = call(b, name)
    assert rc == -1 and "single-output" in msg and "3 output groups" in msg, msg
    assert saved(b) == before


@pytest.mark.parametrize("name", SYMBOLS)
@pytest.mark.parametrize("objective", ["binary:logistic", "count:poisson"])
def test_another_objective_is_refused(name, objective):
    js, _ = S.make_booster(11, 3)
    js = js.replace(b'"name": "reg:squarederror"', b'"name": "' + objective.encode() + b'"')
    assert objective.encode() in js
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    rc, msg = call(b, name)
    assert rc == -1 and name in msg and objective in msg and "reg:squarederror" in msg, msg
    assert saved(b) == before


def _nfeat(js):
    import json
    return int(json.loads(bytes(js).decode())["learner"]["learner_model_param"]["num_feature"])


@pytest.mark.parametrize("name", SYMBOLS)
def test_bad_arguments_are_refused_before_the_matrix_is_looked_at(name):
    js, _ = S.make_booster(11, 3)
    F = _nfeat(js)
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    rc, msg = call(b, name, nfeat=F, labels=False)
    assert rc == -1 and name in msg and "labels is NULL" in msg, msg
    for kw in ({"cut_ptr": False}, {"cut_values": False}):
        rc, msg = call(b, name, nfeat=F, **kw)
        assert rc == -1 and "the cuts are NULL" in msg, msg
    for r in (0, -1):
        rc, msg = call(b, name, nfeat=F, rounds=r)
        assert rc == -1 and "rounds must be >= 1" in msg, msg
    for dep in (0, 9, -3):
        rc, msg = call(b, name, nfeat=F, max_depth=dep)
        assert rc == -1 and "max_depth must be in 1..8" in msg, msg
    for eta in (float("nan"), float("inf"), float("-inf")):
        rc, msg = call(b, name, nfeat=F, eta=eta)
        assert rc == -1 and "eta must be finite" in msg, msg
    for lam in (float("nan"), float("inf"), -1.0, -1e-30):
        rc, msg = call(b, name, nfeat=F, lam=lam)
        assert rc == -1 and "lambda must be finite and >= 0" in msg, msg
        rc, msg = call(b, name, nfeat=F, gamma=lam)
        assert rc == -1 and "gamma must be finite and >= 0" in msg, msg
    rc, msg = call(b, name, nfeat=F, min_child_rows=0)
    assert rc == -1 and "min_child_rows must be >= 1" in msg, msg
    # the cuts
    ptr = np.arange(F + 1, dtype=np.uint64)
    good = np.arange(F, dtype=np.float32)
    for bad in (float("nan"), float("inf"), float("-inf")):
        v = good.copy()
        v[1] = bad
        rc, msg = call(b, name, cuts=(ptr, v))
        assert rc == -1 and "feature 1 are not all finite" in msg, msg
    two = np.array([0, 2] + [2] * (F - 1), dtype=np.uint64)
    for pair in ((1.0, 1.0), (2.0, 1.0), (0.0, -0.0)):
        rc, msg = call(b, name, cuts=(two, np.array(pair, np.float32)))
        assert rc == -1 and "feature 0 are not strictly ascending" in msg, msg
    many = np.array([0, 255] + [255] * (F - 1), dtype=np.uint64)
    rc, msg = call(b, name, cuts=(many, np.arange(255, dtype=np.float32)))
    assert rc == -1 and "255 cuts" in msg and "at most 254" in msg, msg
    rc, msg = call(b, name, cuts=(np.array([1] + [1] * F, np.uint64), good))
    assert rc == -1 and "cut_ptr[0] must be 0" in msg, msg
    rc, msg = call(b, name, cuts=(np.array([0, 2, 1] + [2] * (F - 2), np.uint64), good))
    assert rc == -1 and "must not descend" in msg, msg
    # every argument sound (254 cuts and none are both legal): the NULL matrix is what is left to refuse
    full = np.array([0, 254] + [254] * (F - 1), dtype=np.uint64)
    for kw in ({"cuts": (full, np.arange(254, dtype=np.float32))}, {"cuts": (np.zeros(F + 1, np.uint64), good)},
               {"nfeat": F, "eta": -1.0, "lam": 0.0, "gamma": 5.0, "max_depth": 8, "rounds": 7, "min_child_rows": 1 << 40}):
        rc, msg = call(b, name, **kw)
        assert rc == -1 and "DMatrix handle is invalid" in msg, msg
    assert saved(b) == before, "a refusal changed the forest"


@pytest.mark.parametrize("name", SYMBOLS)
def test_more_than_128_features_are_refused(name):
    js = V.random_booster(3, 2, 129, max_depth=3)
    b = capi.Booster(model_buffer=js)
    before = saved(b)
    rc, msg = call(b, name, nfeat=129)
    assert rc == -1 and "129 features" in msg and "128" in msg, msg
    assert saved(b) == before
    rc, msg = call(capi.Booster(model_buffer=V.random_booster(3, 2, 128, max_depth=3)), name, nfeat=128)
    assert rc == -1 and "DMatrix handle is invalid" in msg, msg


def test_a_model_without_trees_gets_as_far_as_the_matrix():
    b = capi.Booster(model_buffer=G.empty_model(3))
    rc, msg = call(b, "OHXBoosterBoostTrees")
    assert rc == -1 and "DMatrix handle is invalid" in msg, msg


# ---- OHXQuantileCuts ----

def _cuts_case(x, missing, max_bins):
    ptr, vals = capi.quantile_cuts(x, missing, max_bins)
    wptr, wvals = G.quantile_cuts(x, missing, max_bins)
    assert np.array_equal(ptr, wptr), (ptr, wptr)
    assert np.array_equal(helpers.bits(vals), helpers.bits(wvals))
    for f in range(x.shape[1]):
        c = vals[int(ptr[f]):int(ptr[f + 1])]
        assert len(c) <= max_bins - 1 and np.all(np.diff(c) > 0) and np.all(np.isfinite(c))
    return ptr, vals


@pytest.mark.parametrize("missing", [float("nan"), -999.0])
@pytest.mark.parametrize("max_bins", [2, 16, 255])
def test_quantile_cuts_against_the_restatement(missing, max_bins):
    rng = np.random.default_rng(max_bins)
    n = 10000
    x = np.zeros((n, 8), dtype=np.float32)
    x[:, 0] = missing                                         # empty
    x[:, 1] = 3.5                                             # constant
    x[:, 2] = rng.integers(0, 2, n) * 2.0 - 1.0               # 2 distinct values
    x[:, 3] = rng.integers(0, max_bins, n)                    # exactly max_bins distinct values (all appear)
    x[:max_bins, 3] = np.arange(max_bins)
    x[:, 4] = np.floor(rng.normal(0, 40, n))                  # heavy duplicates, more than max_bins of them
    x[:, 5] = rng.normal(0, 1, n)
    x[:, 6] = np.where(rng.random(n) < 0.7, 1.0, rng.normal(0, 1, n))     # one value most of the time
    x[:, 7] = rng.normal(0, 1, n)
    x[rng.random(n) < 0.1, 7] = np.nan
    x[rng.random(n) < 0.1, 7] = -999.0
    x[:5, 5] = [np.inf, -np.inf, np.nan, -999.0, np.inf]      # not finite: never a cut
    ptr, vals = _cuts_case(x, missing, max_bins)
    assert ptr[1] == 0 and ptr[2] == 0, "an empty and a constant column have no cuts"
    assert vals[int(ptr[2]):int(ptr[3])].tolist() == [1.0]
    assert ptr[4] - ptr[3] == max_bins - 1
    if max_bins == 255:
        assert ptr[6] - ptr[5] == 254


def test_quantile_cuts_with_a_cap_that_is_too_small():
    lib = capi.load_library()
    x = np.arange(20, dtype=np.float32).reshape(10, 2)
    ptr = np.zeros(3, dtype=np.uint64)
    vals = np.full(18, -7.0, dtype=np.float32)
    needed = C.c_uint64()
    rc = lib.OHXQuantileCuts(x.ctypes.data, 10, 2, float("nan"), 255, ptr.ctypes.data, vals.ctypes.data, 17, C.byref(needed))
    msg = lib.XGBGetLastError().decode()
    assert rc == -1 and needed.value == 18 and "18 cut values are needed" in msg and "holds 17" in msg, msg
    assert vals[17] == -7.0, "a value was written past cap"
    rc = lib.OHXQuantileCuts(x.ctypes.data, 10, 2, float("nan"), 255, ptr.ctypes.data, vals.ctypes.data, 18, C.byref(needed))
    assert rc == 0 and needed.value == 18 and ptr.tolist() == [0, 9, 18]
    for mb in (1, 256, 0):
        rc = lib.OHXQuantileCuts(x.ctypes.data, 10, 2, float("nan"), mb, ptr.ctypes.data, vals.ctypes.data, 18, C.byref(needed))
        assert rc == -1 and "max_bins must be in 2..255" in lib.XGBGetLastError().decode()


# ---- the split choice on injected histograms ----

def _split_case(Gh, Hh, ncuts, lam=1.0, gamma=0.0, mcr=1):
    Gh = np.asarray(Gh, dtype=np.int64)
    Hh = np.asarray(Hh, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(ncuts)]).astype(np.uint64)
    Gp, Hp = int(Gh[0].sum()), int(Hh[0].sum())
    for f in range(len(Gh)):
        assert int(Gh[f].sum()) == Gp and int(Hh[f].sum()) == Hp, "every row is in one bin of every feature"
    got = synth.grow_node_split(Gh, Hh.astype(np.uint64), ptr, Gp, Hp, lam, gamma, mcr)
    want = G.best_split(Gh, Hh, ncuts, Gp, Hp, lam, mcr)
    if want is None:
        assert not got["valid"] and not got["splits"]
        return got
    loss, f, j, dl, GL, HL = want
    assert got["valid"] and (got["feature"], got["j"], got["default_left"]) == (f, j, dl), (got, want)
    assert np.float64(got["loss_chg"]).view(np.uint64) == np.float64(loss).view(np.uint64)
    assert (got["GL"], got["HL"]) == (GL, HL)
    assert got["splits"] == bool(loss > np.float64(np.float32(gamma)))
    return got


def _hist(nfeat):
    return np.zeros((nfeat, 256), np.int64), np.zeros((nfeat, 256), np.int64)


def test_split_a_single_valid_cut():
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = -3 * Q, 2
    Gh[0, 1], Hh[0, 1] = 5 * Q, 3
    got = _split_case(Gh, Hh, [1], lam=0.0)
    assert (got["feature"], got["j"], got["default_left"]) == (0, 0, 0) and got["splits"]
    # by hand: 9/2 + 25/3 - 4/5
    assert got["loss_chg"] == (4.5 + 25.0 / 3.0) - 0.8


def test_split_missing_rows_decide_the_default():
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = -4 * Q, 4
    Gh[0, 1], Hh[0, 1] = 4 * Q, 4
    Gh[0, 255], Hh[0, 255] = -2 * Q, 2            # the missing rows look like the left ones
    assert _split_case(Gh, Hh, [1])["default_left"] == 1
    Gh[0, 255] = 2 * Q
    assert _split_case(Gh, Hh, [1])["default_left"] == 0
    Gh[0, 255], Hh[0, 255] = 0, 0                 # no missing rows: both defaults tie, dl = 0 by the tie rule
    assert _split_case(Gh, Hh, [1])["default_left"] == 0


def test_split_ties_go_to_the_lower_feature_and_the_lower_cut():
    Gh, Hh = _hist(3)
    for f in (1, 2):                              # two identical features behind one that cannot split
        Gh[f, 0], Hh[f, 0] = -4 * Q, 4
        Gh[f, 1], Hh[f, 1] = 4 * Q, 4
    Gh[0, 0], Hh[0, 0] = 0, 8
    got = _split_case(Gh, Hh, [1, 1, 1])
    assert got["feature"] == 1
    # two cuts of equal gain: bins (a, 0, b): cuts 0 and 1 make the same children
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = -4 * Q, 4
    Gh[0, 2], Hh[0, 2] = 4 * Q, 4
    got = _split_case(Gh, Hh, [2])
    assert got["j"] == 0


def test_split_min_child_rows_excludes_the_best_cut():
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = -50 * Q, 1               # the best cut isolates one row
    Gh[0, 1], Hh[0, 1] = 2 * Q, 3
    Gh[0, 2], Hh[0, 2] = 3 * Q, 4
    assert _split_case(Gh, Hh, [2], mcr=1)["j"] == 0
    assert _split_case(Gh, Hh, [2], mcr=2)["j"] == 1
    assert not _split_case(Gh, Hh, [2], mcr=5)["valid"]
    got = _split_case(Gh, Hh, [2], mcr=4)
    assert got["valid"] and got["j"] == 1 and got["HL"] == 4


def test_split_gamma_just_below_and_just_above_the_best_gain():
    Gh, Hh = _hist(1)
    Gh[0, 0], Hh[0, 0] = -3 * Q, 2
    Gh[0, 1], Hh[0, 1] = 5 * Q, 3
    best = np.float32(_split_case(Gh, Hh, [1])["loss_chg"])
    lo, hi = np.nextafter(best, np.float32(0)), np.nextafter(best, np.float32(100))
    assert _split_case(Gh, Hh, [1], gamma=float(lo))["splits"]
    assert not _split_case(Gh, Hh, [1], gamma=float(hi))["splits"]


def test_split_large_sums_and_lambda_zero():
    Gh, Hh = _hist(2)
    big = (1 << 53) + 1
    Gh[0, 0], Hh[0, 0] = big, 1 << 30
    Gh[0, 1], Hh[0, 1] = -big - 2, 1 << 30
    Gh[1, 0], Hh[1, 0] = -2, 1 << 31
    for lam in (0.0, 1.0, 1e-3):
        got = _split_case(Gh, Hh, [1, 1], lam=lam)
        assert got["feature"] == 0 and got["GL"] == big
    rng = np.random.default_rng(1)
    for case in range(30):
        nf = int(rng.integers(1, 6))
        ncuts = rng.integers(0, 255, nf)
        Gh, Hh = _hist(nf)
        n = int(rng.integers(2, 400))
        q = rng.integers(-(1 << 32), 1 << 32, n)
        for f in range(nf):
            b = rng.integers(0, ncuts[f] + 1, n)
            b[rng.random(n) < 0.2] = 255
            np.add.at(Gh[f], b, q)
            np.add.at(Hh[f], b, 1)
        _split_case(Gh, Hh, ncuts, lam=float(rng.choice([0.0, 1.0])), mcr=int(rng.integers(1, 4)))


# ---- the tree assembly ----

def _hand_tree():
    """The tree of the case worked by hand below."""
    x = np.array([[1, 1], [1, 2], [1, 1], [1, 2], [2, 1], [2, 2], [2, 1], [2, 2]], np.float32)
    y = np.array([0, 2, 0, 2, 4, 4, 4, 4], np.float32)
    cuts = (np.array([0, 1, 2], np.uint64), np.array([2, 2], np.float32))
    return x, y, cuts


@pytest.mark.parametrize("fmt", ["json", "ubj", "binary"])
def test_the_assembly_round_trips_through_the_file_formats(fmt):
    x, y, cuts = _hand_tree()
    out = G.boost(np.zeros(8, np.float32), x, float("nan"), y, cuts, 2, rounds=2, max_depth=2, eta=1.0, lam=0.0)
    leaf_root = G.boost(np.zeros(8, np.float32), x, float("nan"), np.zeros(8, np.float32), cuts, 2, max_depth=2)["trees"][0]
    assert len(leaf_root["left"]) == 1, "a root that stays a leaf"
    trees = out["trees"] + [leaf_root]
    js, _ = S.make_booster(11, 2)
    base = synth.convert_model(js, "json")
    old = G.trees_of(base)
    image = base
    for t in trees:
        image = synth.grow_append(image, t, fmt)
    got = G.trees_of(synth.convert_model(image, "json"))
    assert len(got) == len(old) + 3
    for a, b in zip(got, old):
        assert all(np.array_equal(a[k], b[k]) for k in G.ARRAYS)
    for a, t in zip(got[len(old):], trees):
        assert G.same_tree(a, t) is None, G.same_tree(a, t)
    # and a model written from the restatement reloads to the same new trees
    again = G.trees_of(synth.convert_model(G.with_trees(base, trees), "json"))
    for a, t in zip(again[len(old):], trees):
        assert G.same_tree(a, t) is None
    # out of allocation order, or children that do not name their parent: refused
    bad = {k: v.copy() for k, v in trees[0].items()}
    bad["left"][0], bad["right"][0] = 2, 1
    with pytest.raises(Exception, match="allocation order"):
        synth.grow_append(base, bad, fmt)
    bad = {k: v.copy() for k, v in trees[0].items()}
    bad["parent"][1] = 0
    with pytest.raises(Exception, match="do not name it"):
        synth.grow_append(base, bad, fmt)


# ---- the launch plan ----

@pytest.mark.parametrize("nrow", [1, 63, 4097, 1 << 20, 55987200, 1 << 31])
@pytest.mark.parametrize("nfeat", [1, 3, 27, 53, 54, 128])
def test_the_plan(nrow, nfeat):
    cus = 256
    p = synth.grow_plan(nrow, nfeat, nfeat * 254, 8, cus)
    assert p["block_rows"] == 256 and p["hist_block_rows"] == 1024 and p["max_pairs"] == 53 and p["pair_bytes"] == 256 * 12
    assert p["row_blocks"] == min((nrow + 255) // 256, cus * 8) and (p["row_blocks"] - 1) * 256 < nrow
    assert p["bin_lds_bytes"] == nfeat * 254 * 4 <= 160 * 1024
    assert p["bins_bytes"] == nfeat * nrow and p["hist_bytes"] == 128 * nfeat * 256 * 16
    assert len(p["levels"]) == 8
    for d, l in enumerate(p["levels"]):
        assert l["slots"] == 1 << d
        assert l["lds_bytes"] == l["node_group"] * l["feat_group"] * 256 * 12 <= 160 * 1024
        # groups are the contiguous ranges [g * size, min((g + 1) * size, total)): every node and feature exactly once
        for total, size, groups in ((l["slots"], l["node_group"], l["node_groups"]), (nfeat, l["feat_group"], l["feat_groups"])):
            assert size >= 1 and groups * size >= total and (groups - 1) * size < total
        assert l["hist_blocks"] >= 1 and (l["hist_blocks"] - 1) * 1024 < nrow
        assert l["hist_blocks"] * l["node_groups"] * l["feat_groups"] <= max(cus * 2, l["node_groups"] * l["feat_groups"])
        trips = -(-nrow // (l["hist_blocks"] * 1024))
        assert trips * 1024 < 1 << 32, "a block's 32-bit bin count cannot overflow"


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read(), r.stderr


def kernel_body(text, name_part):
    m = re.search(r"^(_Z\w*" + re.escape(name_part) + r"\w*):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, name_part
    return m.group(2)


@pytest.mark.parametrize("kernel", KERNELS)
def test_grow_kernels_have_no_scratch_no_flat_access_and_no_float_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    if "hist" in kernel:
        assert "ds_add_u64" in body and "ds_add_u32" in body, "the block's histogram is added to with LDS integer adds"
        assert "global_atomic_add_x2" in body, "and flushed with 64-bit global integer adds"
    else:
        assert "atomic_add" not in body and "ds_add" not in body
    if "ILi0E" in kernel:
        assert "v_div_scale_f64" in body, "the gain divides in double"
    m = re.search(r"Function Name: \S*" + re.escape(kernel) + r".*?ScratchSize \[bytes/lane\]: (\d+)", report, re.S)
    assert m and int(m.group(1)) == 0, kernel


# ---- the restatement itself ----

def test_the_restatement_on_a_case_worked_by_hand():
    """8 rows, 2 features, depth 2, base 0, eta 1, lambda 0, gamma 0.  Rows (x0, x1, y): (1,1,0) (1,2,2) twice, (2,1,4)
    (2,2,4) twice; one cut at 2 per feature.  g = -y.  Root: G = -20, H = 8, gain 50.  f0: left G = -4, H = 4 (4) and
    right G = -16, H = 4 (64): loss 18.  f1: -8 | -12: 16 + 36 - 50 = 2.  The root splits on f0.  Node 1 (G = -4, H = 4,
    gain 4): f0 has everyone left (invalid); f1: 0 | -4 with H 2 | 2: 0 + 8 - 4 = 4: splits into nodes 3 and 4.  Node 2
    (G = -16, H = 4, gain 64): f1: -8 | -8: 32 + 32 - 64 = 0, not above gamma: a leaf of 4.  Node 3: w = -(0) / 2 = -0.0."""
    x, y, cuts = _hand_tree()
    out = G.boost(np.zeros(8, np.float32), x, float("nan"), y, cuts, 2, rounds=1, max_depth=2, eta=1.0, lam=0.0)
    t = out["trees"][0]
    lb = -(1 << 31)
    assert t["left"].tolist() == [1, 3, -1, -1, -1] and t["right"].tolist() == [2, 4, -1, -1, -1]
    assert t["parent"].tolist() == [-1, 0 + lb, 0, 1 + lb, 1]
    assert t["feature"].tolist() == [0, 1, 0, 0, 0] and t["default_left"].tolist() == [0, 0, 0, 0, 0]
    assert t["value"].tolist() == [2.0, 2.0, 4.0, 0.0, 2.0] and np.signbit(t["value"][3])
    assert t["loss_chg"].tolist() == [18.0, 4.0, 0.0, 0.0, 0.0]
    assert t["sum_hess"].tolist() == [8.0, 4.0, 4.0, 2.0, 2.0]
    assert t["base_weight"].tolist() == [2.5, 1.0, 4.0, 0.0, 2.0]
    assert out["nodes_added"] == 5 and out["pred"].tolist() == y.tolist()
    # a second round finds nothing left to fit: a root that stays a leaf
    out = G.boost(np.zeros(8, np.float32), x, float("nan"), y, cuts, 2, rounds=2, max_depth=2, eta=1.0, lam=0.0)
    assert len(out["trees"][1]["left"]) == 1 and out["nodes_added"] == 6
    # bins: x < c_j exactly when b <= j; a missing column and a missing value are bin 255
    b = G.bin_rows(np.array([[1.0], [2.0], [np.nan], [np.inf], [-np.inf]], np.float32), float("nan"), cuts, 2)
    assert b.tolist() == [[0, 1, 255, 1, 0], [255] * 5]
    with pytest.raises(ValueError):
        G.boost(np.zeros(8, np.float32), x, float("nan"), y + np.float32(300), cuts, 2)
