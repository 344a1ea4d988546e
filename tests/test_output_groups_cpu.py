"""Boosters with several output groups (multi-class, multi-target), what needs no GPU: they load in all three formats,
OHXBoosterGetNumGroups says G, saving and loading keeps tree_info / num_class / num_target, dart, categorical splits and
a tree_info outside [0, G) are still refused, the OH shell's single-output forms refuse such a booster before touching
the device, and the new kernels cross-compile for gfx950 without scratch or flat memory instructions."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import helpers
from tests import output_groups_support as OG

HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["group_finish_kernel", "group_leaf_gather_kernel", "group_block_scatter_kernel"]


def model_fields(image_json):
    doc = json.loads(bytes(image_json))
    lmp = doc["learner"]["learner_model_param"]
    return (doc["learner"]["gradient_booster"]["model"]["tree_info"], int(lmp["num_class"]), int(lmp["num_target"]),
            doc["learner"]["objective"]["name"])


def load(image):
    return capi.Booster(model_buffer=np.frombuffer(bytes(image), dtype=np.uint8).copy())


@pytest.mark.parametrize("G", [2, 3, 37])
@pytest.mark.parametrize("pattern", OG.PATTERNS)
@pytest.mark.parametrize("multi_target", [False, True])
def test_multi_group_boosters_load_and_round_trip_in_every_format(tmp_path, G, pattern, multi_target):
    ntree = 2 * G + 3
    js, _, info = OG.make_multi(100 + G, ntree, G, pattern,
                                objective="reg:squarederror" if multi_target else "multi:softprob",
                                multi_target=multi_target)
    for fmt, suffix in (("json", ".json"), ("binary", ".model"), ("ubj", ".ubj")):
        image = synth.convert_model(js, fmt)
        b = load(image)
        assert b.num_groups == G
        assert b.info()["num_trees"] == ntree
        path = str(tmp_path / ("m" + suffix))
        b.save_model(path)
        back = capi.Booster(path)
        assert back.num_groups == G
        again = synth.convert_model(np.fromfile(path, dtype=np.uint8), "json")
        got_info, num_class, num_target, objective = model_fields(again.tobytes())
        assert got_info == info
        assert (num_class, num_target) == ((0, G) if multi_target else (G, 1))
        assert objective == ("reg:squarederror" if multi_target else "multi:softprob")
        b.free()
        back.free()


def test_single_group_booster_says_one_group(small_model):
    b = capi.Booster(model_buffer=small_model.image)
    assert b.num_groups == 1


def test_num_groups_of_an_empty_booster_is_an_error():
    b = capi.Booster()
    with pytest.raises(capi.OhxError, match="no model"):
        _ = b.num_groups


@pytest.mark.parametrize("bad", [3, -1, 7])
def test_tree_info_outside_the_groups_is_refused(bad):
    js, _, info = OG.make_multi(5, 9, 3, "round_robin")
    doc = json.loads(js)
    doc["learner"]["gradient_booster"]["model"]["tree_info"][4] = bad
    with pytest.raises(capi.OhxError, match="tree_info"):
        load(json.dumps(doc).encode())


def test_a_single_group_booster_with_tree_info_1_is_refused():
    js, _, _ = OG.make_multi(6, 4, 2, "round_robin")
    doc = json.loads(js)
    doc["learner"]["learner_model_param"]["num_class"] = "0"
    with pytest.raises(capi.OhxError, match="not an output group"):
        load(json.dumps(doc).encode())


def test_dart_and_categorical_multi_group_boosters_are_still_refused():
    js, _, _ = OG.make_multi(7, 6, 3, "blocked")
    doc = json.loads(js)
    doc["learner"]["gradient_booster"]["name"] = "dart"
    doc["learner"]["gradient_booster"] = {"name": "dart", "gbtree": doc["learner"]["gradient_booster"],
                                          "weight_drop": [1.0] * 6}
    with pytest.raises(capi.OhxError, match="dart"):
        load(json.dumps(doc).encode())
    doc = json.loads(js)
    t = doc["learner"]["gradient_booster"]["model"]["trees"][2]
    inner = [i for i, l in enumerate(t["left_children"]) if l != -1]
    if inner:
        t["split_type"][inner[0]] = 1
        t["categories_nodes"] = [inner[0]]
        t["categories_segments"] = [0]
        t["categories_sizes"] = [1]
        t["categories"] = [1]
    else:
        pytest.fail("tree 2 of the plan has no split")
    with pytest.raises(capi.OhxError, match="categorical"):
        load(json.dumps(doc).encode())


FIELD_FORMS = ["OHXBoosterPredictFields", "OHXBoosterPredictFieldsDevice", "OHXBoosterPredictContribsFields",
               "OHXBoosterPredictContribsFieldsDevice", "OHXBoosterRun1", "OHXBoosterRun1Device"]


@pytest.mark.parametrize("name", FIELD_FORMS)
def test_the_oh_shell_forms_refuse_several_groups_before_anything_else(name):
    """Refused at the top of the call, before any argument is read or the device is touched: NULL arguments here."""
    js, _, _ = OG.make_multi(8, 6, 3, "round_robin")
    b = load(js)
    lib = b.lib
    fn = getattr(lib, name)
    args = [b.handle]
    for t in fn.argtypes[1:]:
        if t in (C.c_int32, C.c_int64, C.c_uint32, C.c_uint64):
            args.append(0)
        elif t in (C.c_float, C.c_double):
            args.append(0.0)
        else:
            args.append(None)
    assert fn(*args) == -1
    msg = lib.XGBGetLastError().decode()
    assert "single-output" in msg and "3 output groups" in msg, msg


def test_group_predict_semantics_are_in_the_header():
    text = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    assert "OHXBoosterGetNumGroups" in capi.ABI_SYMBOLS
    assert "[nrow][G]" in text and "out_len" in text


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "groups.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "groups.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel_body(text, name_part):
    m = re.search(r"^(_Z\w*" + re.escape(name_part) + r"\w*):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, name_part
    return m.group(2)


@pytest.mark.parametrize("kernel", KERNELS)
def test_group_kernels_have_no_scratch_and_no_flat_access(isa, kernel):
    body = kernel_body(isa, kernel)
    assert "flat_load" not in body and "flat_store" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert "global_store" in body
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0


# ---- the engineered margins of tests/test_gpu_output_groups_edges.py and its softprob bound ----

@pytest.mark.parametrize("G", [2, 3, 5, 64])
def test_the_softprob_bound_holds_for_the_formula_in_float32_on_the_engineered_margins(G):
    """The 8 float32 ulp of the GPU test are not fitted to the device: 1.6.0's formula evaluated in numpy float32 (expf,
    a double sum, a float divisor, a float quotient) stays within 2.5 ulp of the float64 reference taken from the float32
    difference m_g - max, on every engineered difference - ulp by np.spacing, 2**-149 in the denormal range.  What is
    left of the bound is the device's expf."""
    rows = OG.engineered_rows()
    assert (rows[:, 0] < 0).any() and (rows[:, 0] >= 0).any() and not np.isnan(rows).any()
    worst = 0.0
    for diff in OG.DIFFERENCES:
        for top in (0, G - 1):
            _, leaves, step = OG.engineered_booster(G, diff, top)
            m = OG.engineered_margins(leaves, step, rows)
            assert m.dtype == np.float32 and m.shape == (len(rows), G)
            if diff == "signed_zero":
                assert np.all(m == 0) and np.signbit(m).any() and not np.signbit(m).all()
            elif diff == "ulp":
                d = np.unique(m.max(axis=1, keepdims=True) - m)
                assert np.float32(2.0 ** -24) in d                       # one step below 1.0
            elif diff != "0":
                assert np.any(np.isclose((m.max(axis=1, keepdims=True) - m).astype(np.float64), float(diff), rtol=1e-6))
            ref = OG.softprob_reference(m)
            excess = OG.softprob_excess_ulp(OG.softprob_float32(m), ref)
            worst = max(worst, float(excess.max()))
            assert np.all(excess <= 8), (G, diff, top, float(excess.max()))
            assert np.all(np.abs(ref.sum(axis=1) - 1.0) <= 1e-6)
            if diff in (103.9, 104.1, 88.8):
                tiny = ref[(ref > 0) & (ref < 2.0 ** -126)]
                assert len(tiny)                                         # the reference is a denormal float32 there
    print("G %d: numpy float32 within %.3f ulp" % (G, worst))
    assert worst <= 2.5


def test_the_engineered_boosters_load_with_their_groups():
    image, leaves, step = OG.engineered_booster(5, 87.3)
    b = load(image)
    assert b.num_groups == 5 and b.info()["num_trees"] == 6
    b.free()
