"""oracle/xgb_oracle.py:run1_features - the float32 restatement that OH Run1's feature kernels are held to bit for bit -
against float64 arithmetic on the same inputs, at level counts on either side of every switch in launch_feature_prep
(kernels.hip).  A GPU kernel and its restatement could be wrong in the same way (the wrong end of a SUM, a level
dropped); they cannot both be within float32 rounding of float64 and wrong."""
import numpy as np
import pytest

from oracle import xgb_oracle as O
from tests import helpers

U = 2.0 ** -24
KMS = [1, 7, 64, 65, 128, 129, 181]
GRID = (9, 8)


def sums_ok(x, up, dn):
    """SUM(x(1:k)) and SUM(x(k:km)) in float32 against float64: each within km * 2^-24 * SUM(|x|) of the same range."""
    km = x.shape[2]
    x64 = x.astype(np.float64)
    up64, up_abs = np.cumsum(x64, axis=2), np.cumsum(np.abs(x64), axis=2)
    dn64 = np.cumsum(x64[:, :, ::-1], axis=2)[:, :, ::-1]
    dn_abs = np.cumsum(np.abs(x64)[:, :, ::-1], axis=2)[:, :, ::-1]
    return bool(np.all(np.abs(up.astype(np.float64) - up64) <= km * U * up_abs) and
                np.all(np.abs(dn.astype(np.float64) - dn64) <= km * U * dn_abs))


def f32_sums_dropping_the_end(x):
    """Wrong on purpose: SUM(x(1:k-1)) and SUM(x(k:km-1)), float32, from zero."""
    f32 = np.float32
    km = x.shape[2]
    up, dn = np.zeros_like(x), np.zeros_like(x)
    for k in range(km):
        acc = np.zeros(x.shape[:2], f32)
        for kk in range(k):
            acc = (acc + x[:, :, kk]).astype(f32)
        up[:, :, k] = acc
        acc = np.zeros(x.shape[:2], f32)
        for kk in range(k, km - 1):
            acc = (acc + x[:, :, kk]).astype(f32)
        dn[:, :, k] = acc
    return up, dn


def layer_aod64(st):
    """(aod in float64, the bound on its float32 rounding): thickness, a sum of seven, a product - eight roundings."""
    zle = st["zle_bst"].astype(np.float64)
    thick = zle[:, :, :-1] - zle[:, :, 1:]
    sca = [a.astype(np.float64) for a in st["scacoef"]]
    sc, sc_abs = sum(sca), sum(np.abs(a) for a in sca)
    return thick * sc, 8 * U * np.abs(thick) * sc_abs


@pytest.mark.parametrize("km", KMS)
def test_run1_features_against_float64(km):
    st = helpers.run1_state(GRID + (km,), seed=km)
    feat = O.run1_features(st)
    f32 = np.float32
    tauclw, taucli = st["tauclw"], st["taucli"]
    aod = feat["diag_aod"]
    assert np.count_nonzero(tauclw) and np.count_nonzero(taucli) and np.count_nonzero(aod)
    for x, up, dn in ((tauclw, feat["diag_tauclwup"], feat["diag_tauclwdn"]),
                      (taucli, feat["diag_taucliup"], feat["diag_tauclidn"]),
                      (aod, feat["diag_aodup"], feat["diag_aoddn"])):
        assert sums_ok(x, up, dn)
        # the check has teeth: the two ends of a SUM swapped, or its end level dropped, do not pass it
        if km > 1:
            assert not sums_ok(x, dn, up)
        assert not sums_ok(x, *f32_sums_dropping_the_end(x))
    # the booster's fields are these arrays, in the order of OH_GridCompMod.F90:313-339
    for f, name in ((1, "diag_pl_bst"), (15, "diag_tauclwdn"), (16, "diag_tauclidn"), (17, "diag_taucliup"),
                    (18, "diag_tauclwup"), (21, "diag_strato3"), (23, "diag_aodup"), (24, "diag_aoddn")):
        assert feat["fields"][f] is feat[name]
    # the pointwise features
    ple = st["ple_bst"].astype(np.float64)
    pl64 = (ple[:, :, :-1] + ple[:, :, 1:]) * 0.5
    assert np.all(np.abs(feat["diag_pl_bst"] - pl64) <= U * np.abs(pl64))
    ple_mod = st["ple_mod"].astype(np.float64)
    plm64 = (ple_mod[:, :, :-1] + ple_mod[:, :, 1:]) * 0.5
    assert np.all(np.abs(feat["pl_mod"] - plm64) <= U * np.abs(plm64))
    aod64, bound = layer_aod64(st)
    assert np.all(np.abs(aod.astype(np.float64) - aod64) <= bound)
    without_ni, _ = layer_aod64(dict(st, scacoef=st["scacoef"][:6] + [np.zeros_like(st["scacoef"][6])]))
    assert not np.all(np.abs(without_ni - aod64) <= bound)
    o3 = st["gmito3"].astype(np.float64) - st["gmitto3"].astype(np.float64)
    assert np.all(np.abs(feat["diag_strato3"] - o3) <= U * np.abs(o3))
    assert all(a.dtype == f32 for a in feat["fields"])


def test_run1_is_run1_features_then_the_predict(small_model):
    """run1 takes its fields from run1_features unchanged."""
    st = helpers.run1_state((5, 4, 30), seed=2)
    got = O.run1(O.load_model(small_model.image.tobytes()), st, True)
    feat = O.run1_features(st)
    assert len(got["fields"]) == 27
    for a, b in zip(got["fields"], feat["fields"]):
        assert np.array_equal(helpers.bits(a), helpers.bits(b))
