"""Quantile cuts from rows in HBM, what can be checked without a GPU: the entry point is declared, bound and exported;
every refusal that needs no device, with its message; the radix select itself through its host driver
(synth.quantile_cuts_select: the counting in a plain loop, the step between passes and the final assembly are the code the
product library runs) against the numpy restatement of the header (tests/grow_support.quantile_cuts), for the device's
digits and for others; the key; a case worked by hand; the launch plan; and the kernels cross-compile for gfx950 with no
scratch, no flat memory instruction, no float atomic and no compare-and-swap."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import cuts_support as CS
from tests import helpers

HIPCC = "/opt/rocm/bin/hipcc"
NAME = "OHXDMatrixQuantileCuts"
KERNELS = ["cuts_hist_kernelILi1E", "cuts_hist_kernelILi2E", "cuts_hist_kernelILi3E", "cuts_select_kernelILi1E",
           "cuts_select_kernelILi2E", "cuts_select_kernelILi3E"]
NAN = float("nan")


def test_entry_point_declared_bound_and_exported():
    lib = C.CDLL(helpers.PRODUCT_SO)
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    f90 = open(os.path.join(helpers.ROOT, "quickchem_amd", "fortran", "ohx_bindings.F90")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", helpers.PRODUCT_SO], stdout=subprocess.PIPE, text=True).stdout
    assert NAME in capi.ABI_SYMBOLS
    assert re.search(r"\bint " + NAME + r"\(", header)
    assert hasattr(lib, NAME) and re.search(r" T " + NAME + r"$", nm, re.M)
    assert f'bind(C, name="{NAME}")' in f90
    # behind the host form
    assert header.index("int OHXQuantileCuts(") < header.index("int " + NAME + "(")
    assert f90.index('name="OHXQuantileCuts"') < f90.index(f'name="{NAME}"')
    assert hasattr(capi.DMatrix, "quantile_cuts")
    for fn in ("quantile_cuts_select", "cuts_plan", "cuts_keys"):
        assert hasattr(synth, fn)
    # the host driver is test support: the product exports the one new symbol and nothing else (tests/test_abi.py)
    assert "ohx_cuts" not in nm


def test_the_header_states_the_semantics():
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    header = re.sub(r"\s*\n \*\s*", " ", header)          # comment lines joined
    for phrase in ("rows 0, row_step, 2 * row_step, ... (< nrow)", "the matrix's own `missing`", "apply word for word",
                   "*needed still set", "a cut equal to zero is always +0.0f", "the same predicate",
                   "the caller repeats the last one", "nrow == 0 succeeds with every pointer 0 and launches nothing",
                   "Integer adds only", "no compare-and-swap loops", "nor the matrix form", "waits once, at the end",
                   "not capturable", "freed before it returns", "never a booster's buffer", "max_bins outside 2..255",
                   "row_step < 1", "more than 2^31 rows", "no CPU fallback", "the message says the bytes"):
        assert phrase in header, phrase


def test_refusals_that_need_no_device():
    """The arguments are looked at before the matrix: with every argument sound the NULL matrix is what is left."""
    lib = capi.load_library()
    ptr = np.full(4, 77, dtype=np.uint64)
    vals = np.full(8, -7.0, dtype=np.float32)
    needed = C.c_uint64(12345)

    def call(**kw):
        a = {"row_step": 1, "max_bins": 16, "ptr": ptr.ctypes.data, "vals": vals.ctypes.data, "cap": 8,
             "needed": C.byref(needed)}
        a.update(kw)
        rc = lib.OHXDMatrixQuantileCuts(a.get("d"), a["row_step"], a["max_bins"], a["ptr"], a["vals"], a["cap"], a["needed"], None)
        assert np.all(ptr == 77) and np.all(vals == -7.0) and needed.value == 12345, "a refused call wrote"
        return rc, lib.XGBGetLastError().decode()

    for kw, part in (({"ptr": None}, "NULL output argument"), ({"needed": None}, "NULL output argument"),
                     ({"vals": None}, "cut_values is NULL"), ({"max_bins": 1}, "max_bins must be in 2..255"),
                     ({"max_bins": 256}, "max_bins must be in 2..255"), ({"max_bins": 0}, "max_bins must be in 2..255"),
                     ({"max_bins": -5}, "max_bins must be in 2..255"), ({"row_step": 0}, "row_step must be >= 1"),
                     ({}, "DMatrix handle is invalid"), ({"vals": None, "cap": 0}, "DMatrix handle is invalid"),
                     ({"max_bins": 2}, "DMatrix handle is invalid"), ({"max_bins": 255, "row_step": 1 << 40}, "DMatrix handle is invalid")):
        rc, msg = call(**kw)
        assert rc == -1 and (NAME in msg or "DMatrix handle" in msg), (kw, msg)
        assert part in msg, (kw, msg)
    junk = C.create_string_buffer(b"\x4f" * 256)
    rc, msg = call(d=C.cast(junk, C.c_void_p))
    assert rc == -1 and "DMatrix handle is invalid" in msg, msg


# ---- the select against the restatement ----

@pytest.mark.parametrize("missing", [NAN, -999.0])
@pytest.mark.parametrize("max_bins", [2, 3, 64, 255])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 4097])
def test_the_select_against_the_restatement(n, max_bins, missing):
    x = CS.columns(n, max_bins, missing)
    for step in (1, 3, n + 1):
        CS.same_cuts(synth.quantile_cuts_select(x, missing, max_bins, step), x[::step], missing, max_bins, (n, max_bins, step))


def test_what_the_columns_are():
    """The kinds do what their names say, so that the cases above are the cases meant."""
    x = CS.columns(4097, 64, -999.0)
    k = {name: i for i, name in enumerate(CS.KINDS)}
    low = helpers.bits(x[:, k["low mantissa bits"]])
    assert len(np.unique(low >> 10)) == 1 and len(np.unique(low)) > 64
    z = helpers.bits(x[:, k["zeros of both signs"]])
    assert np.any(z == 0) and np.any(z == 0x80000000)
    den = x[:, k["denormals"]]
    assert np.all(np.abs(den) < np.finfo(np.float32).tiny) and np.any(den < 0) and np.any(den > 0)
    assert len(np.unique(x[:, k["max_bins distinct"]])) == 64 and len(np.unique(x[:, k["max_bins + 1 distinct"]])) == 65
    mixed = x[:, k["nan, -999 and inf mixed"]]
    assert np.any(np.isnan(mixed)) and np.any(mixed == -999.0) and np.any(np.isposinf(mixed)) and np.any(np.isneginf(mixed))
    assert 0.55 < np.mean(x[:, k["60 % zeros"]] == 0) < 0.65
    ptr, vals = synth.quantile_cuts_select(x, -999.0, 64)
    counts = np.diff(ptr.astype(np.int64))
    assert counts[k["constant"]] == 0 and counts[k["all missing"]] == 0
    assert counts[k["max_bins distinct"]] == 63 and counts[k["low mantissa bits"]] == 63


@pytest.mark.parametrize("bits", [(8, 8, 8, 8), (16, 16), (12, 10, 10), (16, 8, 8), (4,) * 8])
def test_the_result_does_not_depend_on_the_digits(bits):
    for n, max_bins, missing, step in ((4097, 64, NAN, 1), (300, 255, -999.0, 1), (65, 2, NAN, 3), (256, 3, -999.0, 1)):
        x = CS.columns(n, max_bins, missing)
        got = synth.quantile_cuts_select(x, missing, max_bins, step, bits)
        CS.same_cuts(got, x[::step], missing, max_bins, (bits, n, max_bins))
        want = synth.quantile_cuts_select(x, missing, max_bins, step)
        assert np.array_equal(got[0], want[0]) and np.array_equal(helpers.bits(got[1]), helpers.bits(want[1]))


def test_digits_that_do_not_sum_to_32_are_refused():
    x = np.zeros((4, 1), dtype=np.float32)
    for bits in ((12, 10), (16, 16, 1), (17, 15), ()):
        with pytest.raises(capi.OhxError):
            synth.quantile_cuts_select(x, NAN, 4, 1, bits)
    with pytest.raises(capi.OhxError, match="max_bins"):
        synth.quantile_cuts_select(x, NAN, 256)
    with pytest.raises(capi.OhxError, match="row_step"):
        synth.quantile_cuts_select(x, NAN, 4, 0)


def test_the_key_round_trips_and_keeps_the_order():
    fmax = np.finfo(np.float32).max
    hand = np.array([-fmax, -1.5, -1.0, -np.finfo(np.float32).tiny, -2.8e-45, -1.4e-45, -0.0, 0.0, 1.4e-45, 2.8e-45,
                     np.finfo(np.float32).tiny, 1.0, 1.5, fmax], dtype=np.float32)
    u = helpers.bits(hand)
    assert u[6] == 0x80000000 and u[7] == 0 and u[8] == 1 and u[5] == 0x80000001, "the list holds both zeros and the smallest denormals"
    keys, back = synth.cuts_keys(u)
    assert keys[6] == keys[7], "both zeros have one key"
    order = np.delete(keys, 6).astype(np.int64)
    assert np.all(np.diff(order) > 0), "the key ascends with the float"
    assert back[6] == 0, "a zero comes back as +0.0f"
    assert np.array_equal(np.delete(back, 6), np.delete(u, 6)), "every other float comes back bit for bit"
    # and on many: every finite float's key orders as the float does
    rng = np.random.default_rng(0)
    r = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    f = r.view(np.float32)
    r = r[np.isfinite(f)]
    f = r.view(np.float32)
    keys, back = synth.cuts_keys(r)
    o = np.argsort(keys, kind="stable")
    assert np.all(np.diff(f[o]) >= 0)
    assert np.array_equal(back[r != 0x80000000], r[r != 0x80000000])


def test_a_case_worked_by_hand():
    """6 rows, 2 columns, max_bins 3, missing NaN.
    Column 0: 5 1 3 1 9 7 -> s = 1 1 3 5 7 9, n = 6, m = 5 > 3: rule (4), s[floor(1 * 6 / 3)] = s[2] = 3 and
    s[floor(2 * 6 / 3)] = s[4] = 7; neither is u_0 = 1: cuts 3, 7.
    Column 1: -2 NaN -2 4 -0.0 0.0 -> s = -2 -2 0 0 4 (the zeros in either order), m = 3 <= 3: rule (3), cuts u_1, u_2 =
    0, 4 - and the zero is +0.0f whichever zero the sort put first.
    With row_step 2 the sample is rows 0, 2, 4: column 0 is 5 3 9 (m = 3): cuts 5, 9; column 1 is -2 -2 -0.0 (m = 2): one
    cut, 0, and it is +0.0f though the only zero in the sample is negative."""
    x = np.array([[5, -2], [1, np.nan], [3, -2], [1, 4], [9, -0.0], [7, 0.0]], dtype=np.float32)
    ptr, vals = synth.quantile_cuts_select(x, NAN, 3)
    assert ptr.tolist() == [0, 2, 4] and vals.tolist() == [3.0, 7.0, 0.0, 4.0]
    assert helpers.bits(vals)[2] == 0
    CS.same_cuts((ptr, vals), x, NAN, 3)
    ptr, vals = synth.quantile_cuts_select(x, NAN, 3, 2)
    assert ptr.tolist() == [0, 2, 3] and vals.tolist() == [5.0, 9.0, 0.0]
    assert helpers.bits(vals)[2] == 0
    CS.same_cuts((ptr, vals), x[::2], NAN, 3)
    # the host form on the same sample agrees but for the sign of that zero
    hptr, hvals = capi.quantile_cuts(x[::2], NAN, 3)
    assert np.array_equal(hptr, ptr) and np.array_equal(hvals, vals)


# ---- the launch plan ----

@pytest.mark.parametrize("nrow", [1, 63, 1024, 1025, 4097, 1 << 20, 55987200, 1 << 31])
@pytest.mark.parametrize("ncol", [1, 3, 10, 11, 27, 128])
def test_the_plan(nrow, ncol):
    cus = 256
    for step in (1, 53, nrow + 1):
        p = synth.cuts_plan(nrow, step, ncol, cus)
        assert p["sampled"] == len(range(0, nrow, step)) and p["block_rows"] == 1024
        want = -(-p["sampled"] // 1024)
        # groups are the contiguous ranges [g * size, min((g + 1) * size, ncol)): every column exactly once
        for size, groups, most in ((p["col_group1"], p["col_groups1"], 10), (p["col_group"], p["col_groups"], 128)):
            assert 1 <= size <= most and groups * size >= ncol and (groups - 1) * size < ncol
        assert p["lds1_bytes"] == p["col_group1"] * 4096 * 4 <= 160 * 1024
        assert p["lds_bytes"] == p["col_group"] * 255 * 4 <= 160 * 1024
        # about two blocks per CU over all of gridDim.y, and never more blocks than there are rows for
        for blocks, groups in ((p["blocks1"], p["col_groups1"]), (p["blocks"], p["col_groups"])):
            assert 1 <= blocks <= want and blocks * groups <= max(2 * cus, groups)
            assert blocks == min(want, max(1, 2 * cus // groups))
            trips = -(-p["sampled"] // (blocks * 1024))
            assert trips * 1024 < 1 << 32, "a block's 32-bit LDS counter cannot overflow"
        assert p["table1_bytes"] == ncol * 4096 * 4 and p["table_bytes"] == ncol * 255 * 1024 * 4
    with pytest.raises(capi.OhxError, match="row_step"):
        synth.cuts_plan(nrow, 0, ncol, cus)


# ---- the kernels cross-compile ----

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "cuts.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "cuts.hip")
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
def test_cuts_kernels_have_no_scratch_no_flat_access_no_float_atomics_and_no_compare_and_swap(isa, kernel):
    text, report = isa
    body = kernel_body(text, kernel)
    assert "flat_load" not in body and "flat_store" not in body and "flat_atomic" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0
    assert not re.search(r"atomic\w*_f(16|32|64)|atomic_pk_add|ds_add\w*_f(32|64)|ds_pk_add", body), "a float atomic"
    assert "cmpswap" not in body and "cmpst" not in body
    if "hist_kernelILi1E" in kernel:
        assert "ds_add_u32" in body, "the block's histogram is added to with LDS integer adds"
        assert "global_atomic_add" in body and "global_atomic_add_x2" not in body, "and flushed with 32-bit global adds"
    elif "hist" in kernel:
        assert "global_atomic_add" in body and "ds_add" not in body
    else:
        assert "atomic_add" not in body and "ds_add" not in body
    if "hist" in kernel:
        assert "v_readlane_b32" in body or "ds_bpermute_b32" in body or "v_readfirstlane_b32" in body, \
            "a wave looks whether its lanes hit one counter"
    m = re.search(r"Function Name: \S*" + re.escape(kernel) + r".*?ScratchSize \[bytes/lane\]: (\d+)", report, re.S)
    assert m and int(m.group(1)) == 0, kernel
