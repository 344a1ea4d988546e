"""Probe for a real libxgboost on boosters with categorical splits (as tests/test_libxgboost_probe.py for the rest): the
routing table of include/ohxgb.h restates common::Decision / GetNextNode<has_missing, has_categorical> of xgboost 1.6.0
and is unpinned until a real library has walked the same model.  Where OHX_LIBXGBOOST names one (1.6.0 is what the
reference pins) these tests compare, bit for bit, its margins and leaf ids on a categorical model - edge values at the
categorical nodes included - with the numpy restatement (CPU) and with the HIP path (-m gpu).  Otherwise they SKIP and
say which variable to set.  The CPU oracle (oracle/) does not know categorical splits and takes no part."""
import numpy as np
import pytest

from oracle import real_xgboost
from quickchem_amd import capi, synth
from tests import categorical_support as CS
from tests import helpers


@pytest.fixture(scope="module")
def real():
    lib, where = real_xgboost.find_libxgboost()
    if lib is None:
        pytest.skip(f"NO REAL libxgboost ON THIS MACHINE - CATEGORICAL ROUTING STAYS UNPINNED (set "
                    f"OHX_LIBXGBOOST=/path/to/libxgboost.so of xgboost 1.6.0 to pin it).  Looked for: {where}")
    print(f"\nreal libxgboost {real_xgboost.version_of(lib)} at {where} (the reference pins 1.6.0 EXACT)")
    return lib


def _case():
    js, trees, cat_max = CS.make_booster(606, 12)
    rows = np.concatenate([CS.rows(607, 5000, cat_max), CS.edge_rows(608, cat_max)])
    return js, trees, cat_max, np.ascontiguousarray(rows, dtype=np.float32)


def _real_predict(lib, path, rows, option_mask):
    b = capi.Booster(lib=lib)
    b.load_model(path)
    d = capi.DMatrix(rows, missing=float("nan"), lib=lib)
    out = b.predict(d, option_mask=option_mask)
    d.free()
    return out


@pytest.mark.parametrize("fmt", ["json", "ubj"])
def test_real_libxgboost_against_the_restatement(real, tmp_path, fmt):
    js, trees, cat_max, rows = _case()
    path = tmp_path / ("categorical." + fmt)
    path.write_bytes(synth.convert_model(js, fmt).tobytes())                 # written by the product's writer
    margins, leaves = CS.predict(trees, CS.base_of(js), rows)
    assert np.array_equal(helpers.bits(_real_predict(real, str(path), rows, 1)), helpers.bits(margins))
    assert np.array_equal(_real_predict(real, str(path), rows, 16).reshape(leaves.shape), leaves)


@pytest.mark.gpu
def test_real_libxgboost_against_the_hip_path(real, tmp_path):
    import torch
    assert torch.cuda.is_available()
    js, trees, cat_max, rows = _case()
    path = tmp_path / "categorical.json"
    path.write_bytes(synth.convert_model(js, "json").tobytes())
    want = _real_predict(real, str(path), rows, 1)
    want_leaves = _real_predict(real, str(path), rows, 16)
    for cat_kernel in ("auto", "direct"):
        b = capi.Booster(str(path))
        b.set_param("ohx_cat_kernel", cat_kernel)
        d = capi.DMatrix(rows, missing=float("nan"))
        assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want)), cat_kernel
        assert np.array_equal(b.predict(d, option_mask=16), want_leaves), cat_kernel
        d.free()
        b.free()


def test_the_probe_names_the_variable_when_it_skips():
    lib, where = real_xgboost.find_libxgboost()
    assert lib is not None or "xgboost" in where
