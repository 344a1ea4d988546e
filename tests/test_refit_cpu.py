"""The leaf refit, what can be checked without a GPU: the two entry points are declared, bound and exported; every
refusal that needs no device, with its message; the solve on injected sums, the write-back through the leaf maps and
the launch plan through libohx_synth.so (the same functions of csrc/refit.cpp the product runs); the three kernels
cross-compile for gfx950 with no scratch and no flat memory instructions; and the numpy restatement the GPU tests
compare against (tests/refit_support.py) is itself held to the derived bound they use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import categorical_support as CS
from tests import helpers
from tests import output_groups_support as OG
from tests import refit_support as R
from tests import visits_support as V

HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["OHXBoosterRefitLeaves", "OHXBoosterRefitLeavesDevice"]
KERNELS = ["refit_leaf_ids_kernelILb1E", "refit_leaf_ids_kernelILb0E", "refit_accumulate_kernel", "refit_solve_kernel"]


def call(b, name, dmat=None, labels=True, nlabel=4, eta=1.0, lam=1.0, unvisited=0):
    """-> (rc, message).  labels: True = four floats on the host."""
    y = np.zeros(4, dtype=np.float32)
    n = C.c_uint64(12345)
    args = [b.handle, dmat, y.ctypes.data if labels else None, nlabel, eta, lam, unvisited, C.byref(n)]
    if name.endswith("Device"):
        args.append(None)
    rc = getattr(b.lib, name)(*args)
    assert rc == 0 or n.value == 12345, "a refused call wrote leaves_refit"
    return rc, b.lib.XGBGetLastError().decode()


def test_entry_points_declared_bound_and_exported():
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
    # after the visit-count block
    assert header.index("int OHXBoosterRefreshCover(") < header.index("int OHXBoosterRefitLeaves(")
    for method in ("refit_leaves", "refit_leaves_device"):
        assert hasattr(capi.Booster, method)
    # interface blocks only: the oracle-linked drivers link ohx_bindings.o and have no such symbols to resolve
    obj = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "obj", "ohx_bindings.o")
    und = subprocess.run(["nm", "--undefined-only", obj], stdout=subprocess.PIPE, text=True).stdout
    assert "RefitLeaves" not in und


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    header = re.sub(r"\s*\n \*\s*", " ", header)          # comment lines joined
    for phrase in ("refresh_leaf = 1", "rint(g * 2^24)", "nearest even", "no float atomics",
                   "-((double)G_l * 2^-24) / ((double)H_l + (double)lambda)", "no fused multiply-add",
                   "unvisited = 0 keeps", "+0.0f in both", "|g| >= 256", "All or nothing", "T * nrow * 4",
                   "Both forms wait", "\"ohx_device\" move"):
        assert phrase in header, phrase


# ---- refusals that need no device ----

@pytest.mark.parametrize("name", SYMBOLS)
def test_no_model_is_refused(name):
    rc, msg = call(capi.Booster(), name)
    assert rc == -1 and "holds no model" in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
def test_a_categorical_booster_is_refused_at_the_top(name):
    js, _, _ = CS.make_booster(5, 3)
    rc, msg = call(capi.Booster(model_buffer=js), name)
    assert rc == -1 and "categorical" in msg and name in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
def test_several_output_groups_are_refused_at_the_top(name):
    js, _, _ = OG.make_multi(8, 6, 3, "round_robin")
    rc, msg = call(capi.Booster(model_buffer=js), name)
    assert rc == -1 and "single-output" in msg and "3 output groups" in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
@pytest.mark.parametrize("objective", ["binary:logistic", "reg:logistic", "count:poisson"])
def test_another_objective_is_refused(name, objective):
    js, _ = S.make_booster(11, 3)
    js = js.replace(b'"name": "reg:squarederror"', b'"name": "' + objective.encode() + b'"')
    assert objective.encode() in js
    rc, msg = call(capi.Booster(model_buffer=js), name)
    assert rc == -1 and name in msg and objective in msg and "reg:squarederror" in msg, msg


@pytest.mark.parametrize("name", SYMBOLS)
def test_bad_arguments_are_refused_before_the_matrix_is_looked_at(name):
    js, _ = S.make_booster(11, 3)
    b = capi.Booster(model_buffer=js)
    before = leaves_now(b)
    rc, msg = call(b, name, labels=False)
    assert rc == -1 and name in msg and "labels is NULL" in msg, msg
    for eta in (float("nan"), float("inf"), float("-inf")):
        rc, msg = call(b, name, eta=eta)
        assert rc == -1 and "eta must be finite" in msg, msg
    for lam in (float("nan"), float("inf"), -1.0, -1e-30):
        rc, msg = call(b, name, lam=lam)
        assert rc == -1 and "lambda must be finite and >= 0" in msg, msg
    for u in (-1, 2, 16):
        rc, msg = call(b, name, unvisited=u)
        assert rc == -1 and "unvisited must be 0 (keep) or 1 (zero)" in msg, msg
    # every argument sound: the NULL matrix is what is left to refuse
    for eta, lam, u in ((1.0, 1.0, 0), (0.3, 0.0, 1), (-1.0, 0.0, 0), (0.0, 5.0, 1)):
        rc, msg = call(b, name, eta=eta, lam=lam, unvisited=u)
        assert rc == -1 and "DMatrix handle is invalid" in msg, msg
    after = leaves_now(b)
    assert all(np.array_equal(helpers.bits(a), helpers.bits(c)) for a, c in zip(before, after)), "a refusal changed the forest"


def leaves_now(b):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.json")
        b.save_model(path)
        v, w = R.leaves_of(open(path, "rb").read())
    return v + w


# ---- the solve on injected sums ----

def _solve_case(G, H, eta, lam, unvisited):
    G = np.asarray(G, dtype=np.int64)
    H = np.asarray(H, dtype=np.uint64)
    rng = np.random.default_rng(len(G))
    old_v = rng.normal(0, 1, len(G)).astype(np.float32)
    old_w = rng.normal(0, 1, len(G)).astype(np.float32)
    v, w, n = synth.refit_solve(G, H, eta, lam, unvisited, old_v, old_w)
    seen = H > 0
    want_v, want_w = old_v.copy(), old_w.copy()
    want_v[seen], want_w[seen] = R.solve(G[seen], H[seen], eta, lam)
    if unvisited:
        want_v[~seen] = 0.0
        want_w[~seen] = 0.0
    assert n == int(seen.sum())
    assert np.array_equal(helpers.bits(v), helpers.bits(want_v)), (eta, lam, unvisited)
    assert np.array_equal(helpers.bits(w), helpers.bits(want_w)), (eta, lam, unvisited)
    return v, w


@pytest.mark.parametrize("unvisited", [0, 1])
@pytest.mark.parametrize("eta", [1.0, 0.3])
@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_the_solve_is_numpy_float64_then_float32(lam, eta, unvisited):
    """Positive, negative and cancelling G; H of 1 and past 2^24; |G| past 2^53; unvisited leaves."""
    q = 1 << 24
    G = [3 * q, -3 * q, 0, 5, -5, (1 << 53) + 1, -(1 << 53) - 3, (1 << 62) + 12345, -(1 << 62) - 999, 7 * q + 1,
         123456789, 0, 0, -(255 << 24) * 3]
    H = [1, 1, 2, 1, (1 << 24) + 1, (1 << 24) + 3, 1 << 31, 1 << 31, (1 << 31) - 1, 7, 3, 0, 0, 3]
    v, w = _solve_case(G, H, eta, lam, unvisited)
    # spot values, by hand: one row of g = 3 gives w = -3 / (1 + lambda)
    assert w[0] == np.float32(-3.0 / (1.0 + lam)) and w[1] == np.float32(3.0 / (1.0 + lam))
    assert v[0] == w[0] * np.float32(eta)
    # G == 0 with rows: -0.0 / (H + lambda), a zero of either sign is a zero
    assert w[2] == 0.0 and v[2] == 0.0
    if unvisited:
        assert helpers.bits(v[11:13]).tolist() == [0, 0] and helpers.bits(w[11:13]).tolist() == [0, 0], "+0.0f"
    rng = np.random.default_rng(5)
    G = rng.integers(-(1 << 40), 1 << 40, 500)
    H = rng.integers(0, 1 << 20, 500)
    H[::7] = 0
    _solve_case(G, H, eta, lam, unvisited)


def test_the_leaf_is_w_times_eta_rounded_twice():
    """A case a fused or double-precision w * eta would round differently: w is rounded to float32 first."""
    rng = np.random.default_rng(8)
    G = rng.integers(-(1 << 30), 1 << 30, 4000)
    H = rng.integers(1, 50, 4000)
    v, w, _ = synth.refit_solve(G, H, 0.3, 1.0, 0, np.zeros(4000, np.float32), np.zeros(4000, np.float32))
    once = ((-(G.astype(np.float64) * 2.0 ** -24) / (H + 1.0)) * np.float64(np.float32(0.3))).astype(np.float32)
    assert np.any(helpers.bits(once) != helpers.bits(v)), "the case set cannot tell one rounding from two"
    assert np.array_equal(helpers.bits(v), helpers.bits(w * np.float32(0.3)))


# ---- the write-back ----

def test_the_write_back_on_hand_made_trees():
    """A root leaf, a stump, a chain, and a tree with deleted slots: only the leaves change, each from its own entry."""
    js, leaves = V.hand_booster()
    trees = V.doc_trees(js)
    offs, loff, lnode = synth.visits_layout(js)
    assert [R.leaf_nodes(t) for t in trees] == leaves
    nleaf = int(loff[-1])
    value = np.arange(1, nleaf + 1, dtype=np.float32) * np.float32(0.5)
    bw = -np.arange(1, nleaf + 1, dtype=np.float32)
    old_v, old_w, node_v, node_w = synth.refit_write_back(js, value, bw)
    k = 0
    for t, tree in enumerate(trees):
        want_v = np.asarray(tree["split_conditions"], dtype=np.float32).copy()
        want_w = np.asarray(tree["base_weights"], dtype=np.float32).copy()
        for n in leaves[t]:
            assert old_v[k] == want_v[n] and old_w[k] == want_w[n]
            want_v[n], want_w[n] = value[k], bw[k]
            k += 1
        a, b = int(offs[t]), int(offs[t + 1])
        assert np.array_equal(helpers.bits(node_v[a:b]), helpers.bits(want_v)), t
        assert np.array_equal(helpers.bits(node_w[a:b]), helpers.bits(want_w)), t
    assert k == nleaf == 9
    # the deleted slots of the last tree and every split keep what the file held
    last = node_v[int(offs[3]):]
    assert last[0] == np.float32(0.5) and last[1] == 0.0 and last[2] == 0.0 and last[3:].tolist() == [4.0, 4.5]


def test_the_write_back_on_adversarial_boosters():
    js, _ = S.make_booster(21, 10)
    trees = V.doc_trees(js)
    offs, loff, _ = synth.visits_layout(js)
    rng = np.random.default_rng(4)
    value = rng.normal(0, 1, int(loff[-1])).astype(np.float32)
    bw = rng.normal(0, 1, int(loff[-1])).astype(np.float32)
    old_v, _, node_v, node_w = synth.refit_write_back(js, value, bw)
    assert np.array_equal(helpers.bits(old_v), helpers.bits(R.leaf_tables(js, R.leaves_of(js)[0])))
    for t, tree in enumerate(trees):
        want_v = np.asarray(tree["split_conditions"], dtype=np.float32).copy()
        want_w = np.asarray(tree["base_weights"], dtype=np.float32).copy()
        ln = R.leaf_nodes(tree)
        want_v[ln] = value[int(loff[t]):int(loff[t + 1])]
        want_w[ln] = bw[int(loff[t]):int(loff[t + 1])]
        assert np.array_equal(helpers.bits(node_v[int(offs[t]):int(offs[t + 1])]), helpers.bits(want_v)), t
        assert np.array_equal(helpers.bits(node_w[int(offs[t]):int(offs[t + 1])]), helpers.bits(want_w)), t


# ---- the launch plan ----

@pytest.mark.parametrize("nrow", [1, 63, 64, 65, 255, 256, 257, 4097, 1 << 20, 55987200, 1 << 31])
def test_the_plan_at_several_row_counts(nrow):
    cus = 256
    p = synth.refit_plan(nrow, 27, 100, cus)
    assert p["block_rows"] == 256 and p["ids_blocks_per_cu"] == 4 and p["accum_blocks_per_cu"] == 8
    tiles = (nrow + 63) // 64
    assert p["ids_blocks"] == min((tiles + 3) // 4, cus * 4) and p["ids_blocks"] >= 1
    assert p["accum_blocks"] == min((nrow + 255) // 256, cus * 8) and p["accum_blocks"] >= 1
    assert p["ids_bytes"] == 100 * nrow * 4
    assert p["stage"] and p["lds_bytes"] == 4 * 27 * 64 * 4
    # no block is launched without a tile or a row of its own
    assert (p["ids_blocks"] - 1) * 4 < tiles and (p["accum_blocks"] - 1) * 256 < nrow


def test_the_plan_says_22_gb_for_the_c360_batch():
    assert synth.refit_plan(55987200, 27, 100)["ids_bytes"] == 22394880000


@pytest.mark.parametrize("nfeat,stage", [(1, True), (27, True), (100, True), (128, True), (129, False), (300, False)])
def test_rows_are_staged_by_the_visit_counts_rule(nfeat, stage):
    p = synth.refit_plan(1000, nfeat, 3, 256)
    assert p["stage"] == stage and p["lds_bytes"] == (4 * nfeat * 64 * 4 if stage else 0) and p["lds_bytes"] <= 128 * 1024
    assert p["stage"] == synth.visits_plan(V.random_booster(50 + nfeat, 3, nfeat, max_depth=4))["stage"]


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "refit.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "refit.hip")
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
def test_refit_kernels_have_no_scratch_no_flat_access_and_no_float_atomics(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add", body), "a float atomic"
    assert "cmpswap" not in body
    if "solve" in kernel:
        assert "atomic" not in body and "v_div_scale_f64" in body, "the solve divides in double and adds nothing"
    else:
        assert "global_atomic_add_x2" in body, "the sums are added to with 64-bit integer adds"
    # the compiler's own report says the same
    m = re.search(r"Function Name: \S*" + re.escape(kernel) + r".*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)",
                  report, re.S)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) == 8, kernel


# ---- the restatement itself ----

def test_the_numpy_restatement_meets_the_bound_the_gpu_is_held_to():
    """One stump, eta = 1, lambda = 0, 200 random cases: every leaf within 2^-24 * (1 + |m|) of the float64 mean m of
    -(base - y) over its rows (tests/refit_support.py stump_bound_ratio says where the bound comes from)."""
    rng = np.random.default_rng(2024)
    worst = 0.0
    for case in range(200):
        n = int(rng.integers(1, 400))
        scale = float(rng.choice([1e-3, 0.1, 1.0, 10.0, 100.0]))
        base = float(rng.normal(0, scale))
        js = R.stump(rng.normal(0, 1), base=base)
        x = rng.normal(0, 1, (n, 3)).astype(np.float32)
        y = (rng.normal(0, scale, n) + rng.normal(0, scale)).astype(np.float32)
        y = np.clip(y, base - 250.0, base + 250.0).astype(np.float32)
        out = R.refit(js, x, float("nan"), y, eta=1.0, reg_lambda=0.0)
        worst = max(worst, R.stump_bound_ratio(js, x, y, out["value"][0]))
    print(f"worst |leaf - m| / bound over 200 cases: {worst:.3f}")
    assert 0.0 < worst <= 1.0, worst


def test_the_restatement_on_a_case_worked_by_hand():
    """base 0.5, a stump on x0 < 0: rows -1, -2 | 3 with labels 1.5, 2.5 | 0.25.  Left: g = -1, -2, G = -3 * 2^24,
    H = 2, lambda 1: w = 1; eta 0.5: leaf 0.5.  Right: g = 0.25, H = 1: w = -0.125, leaf -0.0625."""
    js = R.stump(0.0, base=0.5)
    x = np.array([[-1, 0, 0], [-2, 0, 0], [3, 0, 0]], dtype=np.float32)
    out = R.refit(js, x, float("nan"), np.array([1.5, 2.5, 0.25], np.float32), eta=0.5, reg_lambda=1.0)
    assert out["G"][0].tolist() == [0, -3 << 24, 1 << 22] and out["H"][0].tolist() == [0, 2, 1]
    assert out["base_weight"][0].tolist() == [0.0, 1.0, -0.125] and out["value"][0].tolist() == [0.0, 0.5, -0.0625]
    assert out["leaves_refit"] == 2 and out["pred"].tolist() == [1.0, 1.0, 0.4375]
    with pytest.raises(ValueError):
        R.refit(js, x, float("nan"), np.array([1.5, np.nan, 0.25], np.float32))
    with pytest.raises(ValueError):
        R.refit(js, x, float("nan"), np.array([1.5, 256.5, 0.25], np.float32))
