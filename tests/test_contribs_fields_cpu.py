"""Contributions from the fields, what can be checked without a GPU: the new kernels cross-compile for gfx950 with no
scratch and no flat memory instructions, the C entry points are exported, the Fortran driver is built, and the
oracle-linked drivers still link (nothing they link calls the new symbols)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from quickchem_amd import capi
from tests import helpers

HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["contribs_fields_kernelILb1ELb0E", "contribs_fields_kernelILb1ELb1E", "contribs_fields_kernelILb0ELb0E",
           "contribs_fields_kernelILb0ELb1E", "contribs_fields_combine_kernel"]
SYMBOLS = ["OHXBoosterPredictContribsFields", "OHXBoosterPredictContribsFieldsDevice"]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "contribs.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "contribs.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel_body(text, name_part):
    m = re.search(r"^(_Z\w*" + re.escape(name_part) + r"\w*):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, name_part
    return m.group(2)


@pytest.mark.parametrize("kernel", KERNELS)
def test_fields_kernels_have_no_scratch_and_no_flat_access(isa, kernel):
    body = kernel_body(isa, kernel)
    assert "flat_load" not in body and "flat_store" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0


def test_fields_kernels_store_feature_major(isa):
    """The direct kernels store one float per lane and output (global_store_dword), never a row of them."""
    for kernel in ("contribs_fields_kernelILb1ELb0E", "contribs_fields_kernelILb0ELb0E"):
        body = kernel_body(isa, kernel)
        assert "global_store_dword " in body or "global_store_dword\t" in body
        assert not re.search(r"global_store_dwordx[234]", body)


def test_entry_points_declared_bound_and_exported():
    lib = C.CDLL(helpers.PRODUCT_SO)
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name), name
    assert hasattr(capi.Booster, "predict_contribs_fields")
    assert hasattr(capi.Booster, "predict_contribs_fields_device")


def test_fortran_driver_is_built_against_the_product_only():
    exe = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "contribs_fields_driver_hip")
    assert os.path.exists(exe), exe
    out = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True).stdout
    assert "libohxgb.so" in out and "oracle" not in out
    nm = subprocess.run(["nm", "-D", "--undefined-only", exe], stdout=subprocess.PIPE, text=True).stdout
    assert "OHXBoosterPredictContribsFields" in nm


def test_oracle_linked_drivers_still_link():
    """oracle/Makefile links the product's Fortran objects against liboracle_xgb.so, which has no contributions: those
    drivers exist only while nothing they link calls the new symbols."""
    for name in ("oh_mock_driver_oracle", "oh_run1_driver_oracle", "oh_gridcomp_driver_oracle"):
        exe = os.path.join(helpers.ROOT, "oracle", "lib", name)
        assert os.path.exists(exe), exe
        nm = subprocess.run(["nm", "-D", "--undefined-only", exe], stdout=subprocess.PIPE, text=True).stdout
        assert "ContribsFields" not in nm, name
    obj = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "obj", "ohx_bindings.o")
    nm = subprocess.run(["nm", "--undefined-only", obj], stdout=subprocess.PIPE, text=True).stdout
    assert "ContribsFields" not in nm
