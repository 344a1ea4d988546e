"""Boosting with a held-out set, what can be checked without a GPU: the two entry points are declared, bound, exported
and placed; the header states the semantics; every refusal that needs no device, with outputs and saved bytes unchanged;
the comparison of two sums, the stop rule and the RMSE conversion through the host build of the shared functions, against
Python integers; the two kernels cross-compile for gfx950 with no scratch, no flat access, no float atomic and no
compare-and-swap, and add with 64-bit global integer adds; and the restatement (tests/grow_eval_support.py) on the case
worked by hand and on the early-stopping case of the GPU tests."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import grow_eval_support as E
from tests import grow_support as G
from tests import helpers
from tests.test_grow_cpu import _hand_tree, kernel_body, saved

HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["OHXBoosterBoostTreesEval", "OHXBoosterBoostTreesEvalDevice"]
KERNELS = ["grow_sse_kernel", "grow_walk_sse_kernel"]
SENTINEL = 12345


def call(b, name, dmat=None, labels=True, eval_dmat=None, eval_labels=False, eval_nlabel=0, nfeat=3, rounds=2,
         max_depth=3, eta=0.3, lam=1.0, gamma=0.0, min_child_rows=1, patience=0, run=True, best=True, cut_ptr=True):
    """-> (rc, message); asserts that a refused call wrote no output."""
    y = np.zeros(4, dtype=np.float32)
    ptr, vals = np.arange(nfeat + 1, dtype=np.uint64), np.arange(nfeat, dtype=np.float32)
    train = np.full(rounds + 1 if rounds > 0 else 1, -7.0)
    held = train.copy()
    r, k, n = C.c_int32(SENTINEL), C.c_int32(SENTINEL), C.c_uint64(SENTINEL)
    args = [b.handle, dmat, y.ctypes.data if labels else None, 4, eval_dmat, y.ctypes.data if eval_labels else None,
            eval_nlabel, ptr.ctypes.data if cut_ptr else None, vals.ctypes.data, rounds, max_depth, eta, lam, gamma,
            min_child_rows, patience, train.ctypes.data, held.ctypes.data, C.byref(r) if run else None,
            C.byref(k) if best else None, C.byref(n)]
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
        assert header.index("int OHXBoosterBoostTreesDevice(") < header.index("int " + name + "(") < header.index("int OHXQuantileCuts(")
    for method in ("boost_trees_eval", "boost_trees_eval_device"):
        assert hasattr(capi.Booster, method)
    for f in ("boost_eval_stop", "boost_eval_rmse", "boost_eval_compare", "grow_eval_plan"):
        assert hasattr(synth, f)


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    header = re.sub(r"\s*\n \*\s*", " ", header)          # comment lines joined
    for phrase in ("the held-out rows never influence a tree", "S_t = sum_r q_r^2 is an exact integer",
                   "|q| <= 2^32 - 256", "the high 32 bits of each q^2", "Integer adds only",
                   "sqrt( (double)S_t * 2^-48 / (double)n )", "rounded to nearest even",
                   "never on the doubles", "a tie is not an improvement", "t - best >= patience",
                   "trees 1 .. best are appended", "a stated departure from xgboost", "best == 0 is a success that appends nothing",
                   "eval_dmat == NULL means no held-out set", "its own `missing`", "\"eval label\"",
                   "Nothing is enqueued before the last argument check", "Not capturable", "waits once a round"):
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
    # what the plain call refuses, under this call's name
    rc, msg = call(b, name, nfeat=F, labels=False)
    assert rc == -1 and name in msg and "labels is NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, cut_ptr=False)
    assert rc == -1 and "the cuts are NULL" in msg, msg
    rc, msg = call(b, name, nfeat=F, rounds=0)
    assert rc == -1 and "rounds must be >= 1" in msg, msg
    rc, msg = call(b, name, nfeat=F, max_depth=9)
    assert rc == -1 and "max_depth must be in 1..8" in msg, msg
    rc, msg = call(b, name, nfeat=F, eta=float("nan"))
    assert rc == -1 and "eta must be finite" in msg, msg
    rc, msg = call(b, name, nfeat=F, min_child_rows=0)
    assert rc == -1 and "min_child_rows must be >= 1" in msg, msg
    # its own
    for p in (-1, -100):
        rc, msg = call(b, name, nfeat=F, patience=p)
        assert rc == -1 and name in msg and "patience must be >= 0" in msg, msg
    for kw in ({"run": False}, {"best": False}, {"run": False, "best": False}):
        rc, msg = call(b, name, nfeat=F, **kw)
        assert rc == -1 and "rounds_run or best_round is NULL" in msg, msg
    for p in (1, 3):
        rc, msg = call(b, name, nfeat=F, patience=p)
        assert rc == -1 and "needs a held-out matrix" in msg and f"patience {p}" in msg, msg
    for kw in ({"eval_labels": True}, {"eval_nlabel": 4}, {"eval_labels": True, "eval_nlabel": 4}):
        rc, msg = call(b, name, nfeat=F, **kw)
        assert rc == -1 and "without a held-out matrix" in msg, msg
    # a held-out handle without labels (the handle is not looked at yet)
    rc, msg = call(b, name, nfeat=F, eval_dmat=C.c_void_p(0x1000), eval_nlabel=4)
    assert rc == -1 and "eval labels is NULL" in msg, msg
    # an earlier refusal wins over a later one: the order of the plain call, then this call's own
    rc, msg = call(b, name, nfeat=F, rounds=0, patience=-1)
    assert rc == -1 and "rounds must be >= 1" in msg, msg
    # every argument sound: the NULL training matrix is what is left to refuse
    for kw in ({}, {"patience": 0, "rounds": 7, "max_depth": 8}):
        rc, msg = call(b, name, nfeat=F, **kw)
        assert rc == -1 and "DMatrix handle is invalid" in msg, msg
    assert saved(b) == before, "a refusal changed the forest"


# ---- the comparison of two sums ----

def _int(s):
    return (int(s[0]) << 32) + int(s[1])


def test_sums_compare_as_the_exact_integers():
    M = (1 << 32) - 1
    cases = [((5, 7), (5, 8)),                 # differ only in lo
             ((5, M), (6, 0)),                 # differ in hi, lo the other way round
             ((6, 0), (5, M)),
             ((5, 1 << 32), (6, 0)),           # an un-normalised lo that carries: equal
             ((5, (1 << 32) + 1), (6, 0)),     # ... and is larger by one
             ((5, (3 << 32) + 9), (8, 8)),
             ((0, 0), (0, 0)), ((0, 0), (0, 1)),
             ((1 << 62, (1 << 63) + 5), ((1 << 62) + (1 << 31), 5)),
             ((1 << 62, (1 << 63) + 5), ((1 << 62) + (1 << 31), 6))]
    for a, b in cases:
        want = (_int(a) > _int(b)) - (_int(a) < _int(b))
        got, normal = synth.boost_eval_compare(a, b)
        assert got == want, (a, b, got, want)
        assert normal[1] < 1 << 32 and _int(normal) == _int(a), (a, normal)
        assert synth.boost_eval_compare(b, a)[0] == -want


# ---- the stop rule ----

def _pairs(values, spread=False):
    """Integers as (hi, lo) pairs; spread: lo is left un-normalised where hi has something to lend."""
    out = []
    for v in values:
        hi, lo = v >> 32, v & 0xFFFFFFFF
        if spread and hi > 0:
            hi, lo = hi - 1, lo + (1 << 32)
        out.append((hi, lo))
    return out


@pytest.mark.parametrize("spread", [False, True])
def test_the_stop_rule_on_hand_lists(spread):
    B = 1 << 40
    def rule(values, patience):
        got = synth.boost_eval_stop(_pairs(values, spread), patience)
        assert got == E.stop_rule(lambda t: values[t], len(values) - 1, patience), (values, patience)
        return got
    falling = [B + 9, B + 7, B + 5, B + 3]
    assert rule(falling, 0) == (3, 3) and rule(falling, 1) == (3, 3) and rule(falling, 3) == (3, 3)
    # equal sums: a tie is not an improvement
    assert rule([B, B, B, B], 1) == (1, 0)
    assert rule([B, B - 1, B - 1, B - 1, B - 1], 2) == (3, 1)
    assert rule([B, B, B, B], 0) == (3, 0), "without patience every round runs and best stays"
    # an improvement inside the window resets it
    v = [B + 10, B + 5, B + 6, B + 7, B + 4, B + 8, B + 9, B + 9, B + 1]
    assert rule(v, 3) == (7, 4)
    assert rule(v, 1) == (2, 1)
    assert rule(v, 4) == (8, 8)
    assert rule(v, 0) == (8, 8)
    # patience larger than rounds
    assert rule(v, 100) == (8, 8)
    assert rule([B, B + 1, B + 2], 100) == (2, 0)
    # best == 0
    assert rule([B, B + 1, B + 2, B + 3, B + 4], 3) == (3, 0)
    assert rule([B, B + 1], 1) == (1, 0)
    # sums that differ only in lo, only in hi with lo the other way round
    assert rule([(7 << 32) + 5, (7 << 32) + 4, (7 << 32) + 4], 1) == (2, 1)
    assert rule([(7 << 32) + 5, (6 << 32) + 0xFFFFFFFF, (8 << 32) + 0], 1) == (2, 1)
    assert rule([(6 << 32) + 0xFFFFFFFF, (7 << 32) + 0], 1) == (1, 0)
    # a single entry: no round
    assert rule([B], 2) == (0, 0)


def test_the_stop_rule_on_random_lists():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 30))
        base = int(rng.integers(0, 1 << 30)) << int(rng.integers(0, 60))
        values = [base + int(v) for v in rng.integers(0, 6, n)]
        patience = int(rng.integers(0, 6))
        pairs = [(v >> 32, v & 0xFFFFFFFF) for v in values]
        assert synth.boost_eval_stop(pairs, patience) == E.stop_rule(lambda t: values[t], n - 1, patience)


# ---- the RMSE conversion ----

def test_rmse_conversion_against_python_integers():
    cases = [(0, 7), (1, 1), (1, 3), ((1 << 64) - 1, 1), ((1 << 64) - 1, 4097), (1 << 94, 1 << 31), ((1 << 94) + 12345678901, (1 << 31) - 1),
             # 54 and more bits: rounding to 53 bits both ways, and the ties to even
             ((1 << 53) + 1, 3), ((1 << 53) + 3, 3), ((1 << 80) + (1 << 27), 5), ((1 << 80) + (1 << 27) + 1, 5),
             ((1 << 80) + (3 << 27), 5), ((1 << 80) + (3 << 27) - 1, 5), ((1 << 94) - 1, 1 << 31),
             ((1 << 63) * ((1 << 32) - 256) // (1 << 20), 1000)]
    rng = np.random.default_rng(3)
    for _ in range(200):
        cases.append((int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 33)) | int(rng.integers(0, 1 << 20)), int(rng.integers(1, 1 << 31))))
    down = up = 0
    for Sx, n in cases:
        assert Sx < 1 << 95
        want = math.sqrt(float(Sx) * 2.0 ** -48 / n)
        down += int(float(Sx)) < Sx
        up += int(float(Sx)) > Sx
        hi, lo = Sx >> 32, Sx & 0xFFFFFFFF
        got = synth.boost_eval_rmse(hi, lo, n)
        assert got == want, (Sx, n, got, want)
        if hi > 0:     # the same integer, un-normalised
            assert synth.boost_eval_rmse(hi - 1, lo + (1 << 32), n) == want
    assert down > 10 and up > 10, "cases rounded both ways"
    assert synth.boost_eval_rmse(0, 0, 5) == 0.0
    assert synth.boost_eval_rmse(0, 1, 1) == 2.0 ** -24
    assert synth.boost_eval_rmse(0, 1 << 48, 1) == 1.0 and synth.boost_eval_rmse(1 << 16, 0, 1) == 1.0


def test_the_launch_shape():
    for n in (1, 255, 256, 257, 4097, 1 << 20, 1 << 31):
        p = synth.grow_eval_plan(n, 256)
        assert p["block_rows"] == 256 and p["blocks"] == min((n + 255) // 256, 256 * 8) == synth.grow_plan(n, 3, 0, 2, 256)["row_blocks"]
        assert (p["blocks"] - 1) * 256 < n


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "grow_eval.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow_eval.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read(), r.stderr


@pytest.mark.parametrize("kernel", KERNELS)
def test_eval_kernels_have_no_scratch_no_flat_access_no_float_atomics_and_add_in_64_bits(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    assert len(re.findall(r"global_atomic_add_x2", body)) == 2, "one pair of 64-bit global integer adds"
    m = re.search(r"Function Name: \S*" + re.escape(kernel) + r".*?ScratchSize \[bytes/lane\]: (\d+)", report, re.S)
    assert m and int(m.group(1)) == 0, kernel
    lds = re.search(r"Function Name: \S*" + re.escape(kernel) + r".*?LDS Size \[bytes/block\]: (\d+)", report, re.S)
    assert int(lds.group(1)) == (512 * 16 if "walk" in kernel else 0) + 4 * 2 * 8, "16 bytes a node, and the waves' partial sums"


def test_the_grower_kernels_are_untouched_by_name():
    """grow.hip holds the six kernels it held, and none of the metric's."""
    src = open(os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "grow.hip")).read()
    assert sorted(set(re.findall(r"void (grow_\w+_kernel)\(", src))) == sorted(
        ["grow_bin_kernel", "grow_hist_kernel", "grow_split_kernel", "grow_partition_kernel", "grow_leaf_kernel"])
    assert "sse" not in src


# ---- the restatement itself ----

def test_the_restatement_on_the_case_worked_by_hand():
    """The 8 rows of test_grow_cpu's hand case, held out as well.  Base 0: S_0 = sum y^2 * 2^48 = (4 + 4 + 4 * 16) * 2^48.
    Round 1 fits every row (pred == y): S_1 = 0.  Round 2 grows a root leaf of 0: S_2 = 0, a tie.  With patience 1 the run
    stops at 2 and the best round is 1."""
    x, y, cuts = _hand_tree()
    z = np.zeros(8, np.float32)
    kw = dict(max_depth=2, eta=1.0, lam=0.0)
    out = E.boost_eval(z, x, float("nan"), y, cuts, 2, eval_set=(x, float("nan"), y), eval_pred=z, rounds=5, patience=1, **kw)
    assert out["eval_sums"] == [72 << 48, 0, 0] and out["train_sums"] == out["eval_sums"]
    assert (out["rounds_run"], out["best_round"]) == (2, 1)
    assert out["train_rmse"] == [3.0, 0.0, 0.0] and out["eval_rmse"] == [3.0, 0.0, 0.0]
    assert len(out["trees"]) == 1 and out["nodes_added"] == 5 and len(out["all_trees"][1]["left"]) == 1
    # the same through the library's host rule
    assert synth.boost_eval_stop([(s >> 32, s & 0xFFFFFFFF) for s in out["eval_sums"]], 1) == (2, 1)
    assert [synth.boost_eval_rmse(s >> 32, s & 0xFFFFFFFF, 8) for s in out["eval_sums"]] == out["eval_rmse"]
    # patience 0 keeps all five trees; the best round is still 1
    out = E.boost_eval(z, x, float("nan"), y, cuts, 2, eval_set=(x, float("nan"), y), eval_pred=z, rounds=5, patience=0, **kw)
    assert (out["rounds_run"], out["best_round"], len(out["trees"]), out["nodes_added"]) == (5, 1, 5, 9)
    # no held-out set
    out = E.boost_eval(z, x, float("nan"), y, cuts, 2, rounds=2, **kw)
    assert out["eval_rmse"] is None and (out["rounds_run"], out["best_round"]) == (2, 2) and out["train_rmse"] == [3.0, 0.0, 0.0]
    # the float walk agrees with the bins on the rows the tree was grown from, a missing value takes the default, and
    # a column the matrix lacks is missing
    t = out["trees"][0]
    assert E.walk(t, x, float("nan")).tolist() == y.tolist()
    assert E.walk(t, np.array([[np.nan, 1.0], [-999.0, 2.0], [1.0, np.nan]], np.float32), -999.0).tolist() == [4.0, 4.0, 2.0]
    assert E.walk(t, np.array([[1.0], [2.0]], np.float32), float("nan")).tolist() == [2.0, 4.0]
    with pytest.raises(ValueError, match="eval label"):
        E.boost_eval(z, x, float("nan"), y, cuts, 2, eval_set=(x, float("nan"), y + np.float32(300)), eval_pred=z, **kw)


def early_stopping_case():
    """The early-stopping inputs of the GPU test: 3 features N(0, 1), y = sin(2 x0) + 0.5 x1 + noise; 256 training rows
    with noise 0.5, then 4097 held-out rows with noise 0."""
    rng = np.random.default_rng(0)

    def make(n, noise):
        x = rng.normal(size=(n, 3)).astype(np.float32)
        return x, (np.sin(2 * x[:, 0]) + 0.5 * x[:, 1] + noise * rng.normal(size=n)).astype(np.float32)
    xt, yt = make(256, 0.5)
    xe, ye = make(4097, 0.0)
    return xt, yt, xe, ye, G.quantile_cuts(xt, float("nan"), 64)


def test_the_early_stopping_case_has_its_best_round_strictly_inside():
    xt, yt, xe, ye, cuts = early_stopping_case()
    out = E.boost_eval(np.zeros(256, np.float32), xt, float("nan"), yt, cuts, 3, eval_set=(xe, float("nan"), ye),
                       eval_pred=np.zeros(4097, np.float32), rounds=20, patience=3, max_depth=6, eta=0.5, lam=1.0)
    assert 0 < out["best_round"] < out["rounds_run"] < 20
    assert (out["best_round"], out["rounds_run"]) == (4, 7)
    # the curve, as the figures quoted with the case give it to three decimals: down to round 4, then up
    quoted = [0.872, 0.537, 0.393, 0.332, 0.318, 0.323, 0.332, 0.338]
    assert len(out["eval_rmse"]) == 8 and all(abs(v - q) <= 1e-3 for v, q in zip(out["eval_rmse"], quoted)), out["eval_rmse"]
