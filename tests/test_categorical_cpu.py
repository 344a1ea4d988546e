"""Boosters with categorical splits, what needs no GPU (docs/14_categorical.md): they load from JSON and UBJSON and save
back to both, a booster without such a split is written byte for byte as before, everything Forest::validate refuses has
its message, what such a booster cannot do yet is refused at the top of the call, the flattening walked in Python agrees
with the restatement of the routing table, and categorical.hip cross-compiles to the code its design asks for.  The
adversarial builder of tests/categorical_support.py covers what it promises, its sparse restatement is the dense one,
its tie rows sit on the edges they name, and its boosters (the category 2**24 - 1 included) round-trip and flatten."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import categorical_support as CS
from tests import helpers
from tests import output_groups_support as OG

HIPCC = "/opt/rocm/bin/hipcc"


def load(image):
    return capi.Booster(model_buffer=np.frombuffer(bytes(image), dtype=np.uint8).copy())


def document(image):
    return json.loads(bytes(image), parse_constant=lambda s: {"NaN": "NaN", "Infinity": "Inf", "-Infinity": "-Inf"}[s])


@pytest.fixture(scope="module")
def booster():
    return CS.make_booster(11, 12)


def count_splits(trees):
    return sum(sum(t.stype) for t in trees)


# ---------------------------------------------------------------- loading and round trips

def test_the_builder_covers_what_it_promises(booster):
    _, trees, cat_max = booster
    assert sorted(cat_max.values()) == sorted(CS.MAXES)
    seen = {max(c) for t in trees for c in t.cats.values()}
    assert seen == set(CS.MAXES)
    assert {t.depth() for t in trees} >= {1, 18}
    assert trees[0].stype[0] == 1                                                   # a categorical root
    t = trees[1]
    inner = [n for n in range(len(t.left)) if t.left[n] != -1]
    assert {t.stype[n] for n in inner} == {0, 1} and len({t.feat[n] for n in inner}) == 1   # one feature, both ways
    assert {t.dl[n] for t in trees for n in t.cats} == {0, 1}


@pytest.mark.parametrize("fmt", ["json", "ubj"])
def test_loads_and_counts_its_categorical_splits(booster, fmt):
    js, trees, _ = booster
    b = load(synth.convert_model(js, fmt))
    assert b.num_categorical_splits() == count_splits(trees) > 0
    assert b.num_groups == 1
    info = b.info()
    assert info["num_trees"] == len(trees) and info["num_nodes"] == sum(len(t.left) for t in trees)
    b.free()


def test_a_numeric_booster_has_no_categorical_split(small_model):
    b = capi.Booster(model_buffer=small_model.image)
    assert b.num_categorical_splits() == 0


def test_the_count_of_an_empty_booster_is_an_error():
    with pytest.raises(capi.OhxError, match="no model"):
        capi.Booster().num_categorical_splits()


def test_load_save_load_is_identical_in_both_formats_and_across_them(booster, tmp_path):
    js, trees, cat_max = booster
    first = document(synth.convert_model(js, "json"))
    # what the writer makes of the builder's document is the document: every array of the file, NaN conditions included
    want = document(js)
    for key in ("categories", "categories_nodes", "categories_segments", "categories_sizes", "split_type", "split_indices",
                "default_left", "left_children", "right_children"):
        for a, b in zip(first["learner"]["gradient_booster"]["model"]["trees"],
                        want["learner"]["gradient_booster"]["model"]["trees"]):
            assert a[key] == b[key], key
    for t, a in zip(trees, first["learner"]["gradient_booster"]["model"]["trees"]):
        for n in t.cats:
            assert a["split_conditions"][n] == "NaN"
    images = {"json": synth.convert_model(js, "json"), "ubj": synth.convert_model(js, "ubj")}
    for src in ("json", "ubj"):
        for dst, suffix in (("json", ".json"), ("ubj", ".ubj")):
            b = load(images[src])
            path = str(tmp_path / ("m_" + src + suffix))
            b.save_model(path)
            saved = np.fromfile(path, dtype=np.uint8)
            assert bytes(saved) == bytes(images[dst]), (src, dst)                  # save(load(x)) is the writer's x
            back = capi.Booster(path)
            assert back.num_categorical_splits() == count_splits(trees)
            assert document(synth.convert_model(saved, "json")) == first
            b.free()
            back.free()


def test_feature_names_and_types_survive(booster):
    js, _, cat_max = booster
    for fmt in ("json", "ubj"):
        doc = document(synth.convert_model(synth.convert_model(js, fmt), "json"))
        assert doc["learner"]["feature_types"] == ["c" if f in cat_max else "float" for f in range(CS.NFEAT)]
        assert doc["learner"]["feature_names"] == ["f%d" % f for f in range(CS.NFEAT)]


@pytest.mark.parametrize("fmt", ["json", "ubj"])
def test_a_numeric_booster_is_written_byte_for_byte_as_before(fmt):
    """tests/golden/hand_forest_parent_writer.*: hand_forest.json as the writer of the commit before categorical splits
    wrote it."""
    src = np.fromfile(os.path.join(helpers.GOLDEN, "hand_forest.json"), dtype=np.uint8)
    want = np.fromfile(os.path.join(helpers.GOLDEN, "hand_forest_parent_writer." + fmt), dtype=np.uint8)
    assert bytes(synth.convert_model(src, fmt)) == bytes(want)


# ---------------------------------------------------------------- refusals

def test_saving_in_the_legacy_binary_format_is_refused(booster, tmp_path):
    js, _, _ = booster
    b = load(js)
    with pytest.raises(capi.OhxError, match="categorical.*JSON/UBJ"):
        b.save_model(str(tmp_path / "m.model"))
    with pytest.raises(capi.OhxError, match="categorical"):
        synth.convert_model(js, "binary")


def _split_type(t):
    leaf = [i for i, l in enumerate(t["left_children"]) if l == -1][0]
    t["split_type"][leaf] = 1


def _numeric_named(t):
    numeric = [i for i, l in enumerate(t["left_children"]) if l != -1 and t["split_type"][i] == 0]
    t["categories_nodes"][0] = numeric[0]


def _no_segment(t):
    for key in ("categories_nodes", "categories_segments", "categories_sizes"):
        t[key] = t[key][1:]


MUTATIONS = {
    "split_type 2": lambda t: t["split_type"].__setitem__(t["categories_nodes"][0], 2),
    "is a leaf or a deleted slot": _split_type,
    "out of range": lambda t: t["categories_nodes"].__setitem__(0, len(t["left_children"]) + 5),
    "more than once": lambda t: [t[k].append(t[k][0]) for k in ("categories_nodes", "categories_segments", "categories_sizes")],
    "numeric node": _numeric_named,
    "has no segment": _no_segment,
    "size 0": lambda t: t["categories_sizes"].__setitem__(0, 0),
    "runs past categories": lambda t: t["categories_segments"].__setitem__(len(t["categories_segments"]) - 1,
                                                                           len(t["categories"])),
    "negative category": lambda t: t["categories"].__setitem__(0, -1),
    "above the limit": lambda t: t["categories"].__setitem__(0, 2 ** 24),
}


@pytest.mark.parametrize("message", sorted(MUTATIONS))
def test_validate_refuses_with_a_message_of_its_own(message):
    js, _, _ = CS.make_booster(12, 4, depths=[3, 4, 2, 5], p_cat=0.5)
    doc = json.loads(js)
    t = doc["learner"]["gradient_booster"]["model"]["trees"][1]      # tree 1: a categorical root, numeric nodes below
    assert t["categories_nodes"] and any(s == 0 and l != -1 for s, l in zip(t["split_type"], t["left_children"]))
    MUTATIONS[message](t)
    for fmt in ("json", "ubj"):
        image = json.dumps(doc).encode()
        with pytest.raises(capi.OhxError, match=message):
            load(image if fmt == "json" else _to_ubj_unchecked(doc))


def _to_ubj_unchecked(doc):
    """The document as UBJSON written HERE (the product's writer would validate it first): general containers, int64
    and float32 scalars - what the reader must accept beside xgboost's typed arrays."""
    out = bytearray()

    def key(s):
        b = s.encode()
        out.extend(b"L" + struct.pack(">q", len(b)) + b)

    def value(v):
        if isinstance(v, dict):
            out.extend(b"{")
            for k, x in v.items():
                key(k)
                value(x)
            out.extend(b"}")
        elif isinstance(v, list):
            out.extend(b"[")
            for x in v:
                value(x)
            out.extend(b"]")
        elif isinstance(v, str):
            out.extend(b"S")
            key(v)
        elif isinstance(v, bool):
            out.extend(b"T" if v else b"F")
        elif isinstance(v, int):
            out.extend(b"L" + struct.pack(">q", v))
        else:
            out.extend(b"d" + struct.pack(">f", v))
    value(doc)
    return bytes(out)


def test_the_largest_category_the_header_promises_loads():
    js, _, _ = CS.make_booster(13, 1, depths=[1])
    doc = json.loads(js)
    t = doc["learner"]["gradient_booster"]["model"]["trees"][0]
    t["categories"][0] = 2 ** 24 - 1
    b = load(json.dumps(doc).encode())
    assert b.num_categorical_splits() == 1
    header = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    assert "OHX_MAX_CATEGORY 16777215" in header


def test_several_output_groups_with_a_categorical_split_stay_refused():
    js, _, _ = OG.make_multi(7, 6, 3, "blocked")
    doc = json.loads(js)
    t = doc["learner"]["gradient_booster"]["model"]["trees"][2]
    inner = [i for i, l in enumerate(t["left_children"]) if l != -1]
    t["split_type"][inner[0]] = 1
    t["categories_nodes"], t["categories_segments"], t["categories_sizes"], t["categories"] = [inner[0]], [0], [2], [1, 40]
    with pytest.raises(capi.OhxError, match="categorical.*several output groups"):
        load(json.dumps(doc).encode())


REFUSED = ["OHXBoosterPredictFields", "OHXBoosterPredictFieldsDevice", "OHXBoosterPredictContribs",
           "OHXBoosterPredictContribsDevice", "OHXBoosterPredictContribsFields", "OHXBoosterPredictContribsFieldsDevice",
           "OHXBoosterPredictInteractions", "OHXBoosterPredictInteractionsDevice", "OHXBoosterRun1", "OHXBoosterRun1Device"]


@pytest.mark.parametrize("name", REFUSED)
def test_what_a_categorical_booster_cannot_do_is_refused_at_the_top_of_the_call(booster, name):
    """Before any argument is read or the device is touched: every other argument is NULL or 0 here."""
    b = load(booster[0])
    fn = getattr(b.lib, name)
    args = [b.handle]
    for t in fn.argtypes[1:]:
        if t in (C.c_int, C.c_uint, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64):
            args.append(0)
        elif t in (C.c_float, C.c_double):
            args.append(0.0)
        else:
            args.append(None)
    assert fn(*args) == -1
    msg = b.lib.XGBGetLastError().decode()
    assert "categorical" in msg and name in msg, msg


def test_get_info_names_the_new_node_format_for_such_boosters_only(booster, small_model):
    b = load(booster[0])
    flat = synth.cat_flatten_cpu(booster[0])
    arr = (C.c_uint64 * 8)()
    assert b.lib.OHXBoosterGetInfo(b.handle, arr) == 0
    assert arr[6] == 3 and arr[2] == len(flat["nodes"]) and arr[3] == 16 * len(flat["nodes"]) + 4 * len(flat["words"])
    n = capi.Booster(model_buffer=small_model.image)
    assert n.lib.OHXBoosterGetInfo(n.handle, arr) == 0
    assert arr[6] in (0, 1, 2)


def test_the_semantics_are_in_the_header_and_the_binding():
    text = open(os.path.join(helpers.ROOT, "include", "ohxgb.h")).read()
    assert "OHXBoosterGetNumCategoricalSplits" in capi.ABI_SYMBOLS
    assert "tested FIRST" in text and "RIGHT" in text and "32 * ceil((M + 1) / 32)" in text
    f90 = open(os.path.join(helpers.ROOT, "quickchem_amd", "fortran", "ohx_bindings.F90")).read()
    assert 'name="OHXBoosterGetNumCategoricalSplits"' in f90


# ---------------------------------------------------------------- the flattening, walked in Python

K_CAT, K_WORDS, K_FEATURE = 1 << 30, 1 << 29, (1 << 29) - 1


def walk_flat(flat, base, X, missing, pred_leaf=False):
    """The kernels' step (categorical.hip step_right) on emit_cat's arrays, one row at a time."""
    nodes, words, roots = flat["nodes"], flat["words"], flat["roots"]
    as_float = nodes.view(np.float32)
    out = np.zeros((len(X), len(roots)) if pred_leaf else len(X), dtype=np.float32)
    for r, x in enumerate(X):
        acc = np.float32(base)
        for ti, slot in enumerate(roots):
            slot = int(slot)
            while nodes[slot, 1] != 0:
                bits, left, meta = int(nodes[slot, 0]), int(nodes[slot, 1]), int(nodes[slot, 2])
                f = meta & K_FEATURE
                v = np.float32(x[f]) if f < len(x) else np.float32(np.nan)
                if not np.isnan(missing) and v == np.float32(missing):
                    v = np.float32(np.nan)
                dl = (meta >> 31) != 0
                if meta & K_CAT:
                    in_range = bool(v >= 0) and bool(v < as_float[slot, 3])
                    if in_range:
                        c = int(v)
                        word = int(words[bits + (c >> 5)]) if meta & K_WORDS else bits
                        go_left = ((word >> (c & 31)) & 1) == 0
                    else:
                        go_left = dl
                else:
                    go_left = dl if np.isnan(v) else bool(v < as_float[slot, 0])
                slot = left + (0 if go_left else 1)
            if pred_leaf:
                out[r, ti] = flat["orig_id"][slot]
            else:
                acc = np.float32(acc + as_float[slot, 0])
        if not pred_leaf:
            out[r] = acc
    return out


@pytest.mark.parametrize("missing", [np.nan, -999.0])
def test_the_flat_arrays_walked_in_python_agree_with_the_restatement(booster, missing):
    js, trees, cat_max = booster
    flat = synth.cat_flatten_cpu(js)
    assert flat["inline_sets"] > 0 and flat["word_sets"] > 0
    assert flat["inline_sets"] + flat["word_sets"] == count_splits(trees)
    # a set of M < 32 costs no word; the others 32-bit words up to their largest category
    want_words = sum(CS.capacity(max(c)) // 32 for t in trees for c in t.cats.values() if max(c) >= 32)
    assert len(flat["words"]) == want_words
    X = np.concatenate([CS.rows(21, 300, cat_max, missing=missing), CS.edge_rows(22, cat_max, missing=missing)])
    for ncol in (CS.NFEAT, 9):
        margins, leaves = CS.predict(trees, CS.base_of(js), X[:, :ncol], missing)
        got = walk_flat(flat, CS.base_of(js), X[:, :ncol], missing)
        assert np.array_equal(helpers.bits(got), helpers.bits(margins))
        assert np.array_equal(walk_flat(flat, CS.base_of(js), X[:, :ncol], missing, pred_leaf=True), leaves)


# ---------------------------------------------------------------- the adversarial builder (tests/categorical_support.py)

@pytest.fixture(scope="module")
def adversarial():
    return CS.make_adversarial(5150, 33, maxcat=True)


def path_to(t, n):
    par = {c: m for m in range(len(t.left)) if t.left[m] != -1 for c in (t.left[m], t.right[m])}
    out = []
    while n in par:
        n = par[n]
        out.append(n)
    return out[::-1]


def test_the_adversarial_builder_covers_what_it_promises(adversarial):
    _, trees, cat_max = adversarial
    assert {t.kind for t in trees} == set(CS.KINDS) | {"maxcat"}
    assert {k for t in trees for k in t.setkind.values()} == set(CS.SET_KINDS) | {"maxcat"}
    assert max(t.depth() for t in trees) == 30
    for t in trees:
        assert (t.kind == "leaf") == (len(t.left) == 1)
        assert set(t.setkind) == set(t.cats)
    # a root leaf in both positions of a pair, a depth-30 chain beside it
    assert (trees[0].kind, trees[1].depth()) == ("leaf", 30) and (trees[2].depth(), trees[3].kind) == (30, "leaf")
    for ntree, first, second in ((2, 0, 30), (3, 30, 0)):
        _, small, _ = CS.make_adversarial(1, ntree)
        assert (small[0].depth(), small[1].depth()) == (first, second)
    _, one, _ = CS.make_adversarial(1, 1)
    assert len(one) == 1 and one[0].depth() == 30
    assert {len(CS.make_adversarial(1, n)[1]) & 1 for n in (1, 2, 3, 5, 10, 33)} == {0, 1}
    # the set kinds are what their names say
    for t in trees:
        for n, kind in t.setkind.items():
            c = t.cats[n]
            if kind == "zero":
                assert c == [0]
            elif kind == "top":
                assert len(c) == 1
            elif kind == "full":
                assert sorted(c) == list(range(max(c) + 1))
            elif kind == "edges":
                assert set(c) <= set(CS.WORD_EDGES)
            elif kind == "repeated":
                assert len(set(c)) < len(c)
            elif kind == "maxcat":
                assert max(c) == 2 ** 24 - 1 == CS.MAX_CATEGORY and len(c) > 1 and min(c) < 32
    assert {t.cats[n][0] for t in trees for n, k in t.setkind.items() if k == "top"} >= {31, 32, 64, 1000}
    assert any(t.cats[n] != sorted(t.cats[n]) for t in trees for n, k in t.setkind.items() if k == "repeated")
    assert any(set(t.cats[n]) == set(CS.WORD_EDGES) for t in trees for n, k in t.setkind.items() if k == "edges")
    # a chain alternates numeric and categorical splits of ONE feature, its thresholds integers or their neighbours
    for t in trees:
        if t.kind != "chain":
            continue
        inner = [n for n in range(len(t.left)) if t.left[n] != -1]
        assert len({t.feat[n] for n in inner}) == 1 and {t.stype[n] for n in inner} == {0, 1}
        for n in inner:
            if t.stype[n] == 0:
                c = np.float32(t.cond[n])
                k = np.float32(np.round(c))
                assert c in (k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf)))
    assert {np.float32(t.cond[n]) == np.round(np.float32(t.cond[n])) for t in trees if t.kind == "chain"
            for n in range(len(t.left)) if t.left[n] != -1 and t.stype[n] == 0} == {True, False}
    # mixed capacity: on ONE path, one feature with a one-word set above a larger one and the reverse
    orders = set()
    for t in trees:
        if t.kind != "mixed_capacity":
            continue
        deepest = max((n for n in range(len(t.left)) if t.left[n] != -1), key=lambda n: len(path_to(t, n)))
        spine = path_to(t, deepest) + [deepest]
        assert len({t.feat[n] for n in spine}) == 1 and all(t.stype[n] == 1 for n in spine)
        caps = [CS.capacity(max(t.cats[n])) for n in spine]
        assert len(set(caps)) >= 4
        for a, b in zip(caps, caps[1:]):
            if a != b:
                orders.add((a == 32, b == 32))
    assert {(True, False), (False, True)} <= orders
    assert {t.dl[n] for t in trees for n in t.cats} == {0, 1}


def test_category_tie_rows_sit_on_the_edges_they_name(adversarial):
    _, trees, cat_max = adversarial
    X = CS.category_tie_rows(np.random.default_rng(8), trees, 1500, cat_max)
    assert X.dtype == np.float32 and not np.isnan(X).any() and not np.isinf(X).any()
    cat_cols = X[:, sorted(cat_max)]
    assert np.any((cat_cols == 0) & np.signbit(cat_cols))                           # -0.0
    assert np.any(cat_cols == CS.DENORMAL) and np.any(cat_cols == -CS.DENORMAL)
    frac = cat_cols[(cat_cols > 1) & (cat_cols != np.trunc(cat_cols))]
    assert np.any(np.nextafter(frac, np.float32(np.inf)) == np.trunc(frac) + 1)     # just below an integer
    sizes = {np.float32(CS.capacity(max(c))) for t in trees for c in t.cats.values()}
    assert sizes >= {32.0, 64.0, 96.0, 1024.0, 2.0 ** 24}
    for s in (np.float32(32), np.float32(64)):
        assert np.any(cat_cols == s) and np.any(cat_cols == np.nextafter(s, np.float32(0))) and np.any(cat_cols == s - 1)


def test_category_tie_rows_reach_the_last_level_of_every_spine():
    """The rows the GPU tests use: the deepest node of each depth-30 chain and of each mixed-capacity spine is reached
    by some row, both children of every stump, and at least a quarter of every tree's leaves."""
    _, trees, cat_max = CS.make_adversarial(710, 10)
    X = np.concatenate([CS.rows(10, 1200, cat_max, missing=-999.0),
                        CS.category_tie_rows(np.random.default_rng(10), trees, 700, cat_max)])
    _, leaves = CS.predict(trees, 0.0, X, walker=CS.walk_sparse)
    for ti, t in enumerate(trees):
        depth_of = {0: 0}
        for n in range(len(t.left)):
            if t.left[n] != -1:
                depth_of[t.left[n]] = depth_of[t.right[n]] = depth_of[n] + 1
        reached = np.unique(leaves[:, ti]).astype(int)
        nleaf = sum(1 for n in range(len(t.left)) if t.left[n] == -1)
        print("tree %d (%s, depth %d): %d of %d leaves reached" % (ti, t.kind, t.depth(), len(reached), nleaf))
        if t.kind in ("chain", "mixed_capacity", "cat_stump"):
            assert max(depth_of[n] for n in reached) == t.depth()
        if t.kind == "cat_stump":
            assert len(reached) == 2
        assert 4 * len(reached) >= nleaf


def test_the_sparse_restatement_is_the_dense_one(booster):
    """walk_sparse keeps `walk`'s tests in their order and looks membership up in sorted keys: the same leaves on the
    first builder's boosters (and on an adversarial one without the 2**24 - 1 node, whose dense table does not exist)."""
    cases = [booster, CS.make_booster(2024, 12), CS.make_booster(31, 10, suffix=True), CS.make_adversarial(3, 10)]
    for js, trees, cat_max in cases:
        for missing in (np.nan, -999.0):
            X = np.concatenate([CS.rows(21, 400, cat_max, missing=missing), CS.edge_rows(22, cat_max, missing=missing)])
            for ncol in (CS.NFEAT, 9):
                for t in trees:
                    assert np.array_equal(CS.walk(t, X[:, :ncol], missing), CS.walk_sparse(t, X[:, :ncol], missing))
            a = CS.predict(trees, CS.base_of(js), X, missing, 5)
            b = CS.predict(trees, CS.base_of(js), X, missing, 5, walker=CS.walk_sparse)
            assert np.array_equal(helpers.bits(a[0]), helpers.bits(b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("missing", [np.nan, -999.0])
def test_the_flat_arrays_walked_in_python_agree_on_the_adversarial_booster(adversarial, missing):
    js, trees, cat_max = adversarial
    flat = synth.cat_flatten_cpu(js)
    assert flat["inline_sets"] + flat["word_sets"] == count_splits(trees)
    want_words = sum(CS.capacity(max(c)) // 32 for t in trees for c in t.cats.values() if max(c) >= 32)
    assert len(flat["words"]) == want_words >= 2 ** 19                               # the 2**24 - 1 node alone: 524 288
    ties = CS.category_tie_rows(np.random.default_rng(4), trees, 400, cat_max)
    X = np.concatenate([CS.rows(21, 150, cat_max, missing=missing), ties, CS.edge_rows(22, cat_max, missing=missing)])
    X[:6, 1] = np.array([16777215, 16777214, 16777216, 8388607.5, 3e9, np.nan], dtype=np.float32)
    for ncol in (CS.NFEAT, 9):
        margins, leaves = CS.predict(trees, CS.base_of(js), X[:, :ncol], missing, walker=CS.walk_sparse)
        got = walk_flat(flat, CS.base_of(js), X[:, :ncol], missing)
        assert np.array_equal(helpers.bits(got), helpers.bits(margins))
        assert np.array_equal(walk_flat(flat, CS.base_of(js), X[:, :ncol], missing, pred_leaf=True), leaves)


def test_load_save_load_of_the_adversarial_booster(adversarial, tmp_path):
    """JSON and UBJSON, the node with category 2**24 - 1 included; a list with repeated members comes back as the file
    gave it (the writer writes what the reader read, not the set)."""
    js, trees, cat_max = adversarial
    want = document(js)["learner"]["gradient_booster"]["model"]["trees"]
    assert any(2 ** 24 - 1 in t["categories"] for t in want)
    assert any(len(set(c)) < len(c) for t in trees for c in t.cats.values())
    images = {"json": synth.convert_model(js, "json"), "ubj": synth.convert_model(js, "ubj")}
    first = document(images["json"])
    for key in ("categories", "categories_nodes", "categories_segments", "categories_sizes", "split_type", "split_indices",
                "default_left", "left_children", "right_children"):
        for a, b in zip(first["learner"]["gradient_booster"]["model"]["trees"], want):
            assert a[key] == b[key], key
    for src in ("json", "ubj"):
        for dst, suffix in (("json", ".json"), ("ubj", ".ubj")):
            b = load(images[src])
            assert b.num_categorical_splits() == count_splits(trees)
            path = str(tmp_path / ("adv_" + src + suffix))
            b.save_model(path)
            saved = np.fromfile(path, dtype=np.uint8)
            assert bytes(saved) == bytes(images[dst]), (src, dst)
            back = capi.Booster(path)
            assert back.num_categorical_splits() == count_splits(trees)
            assert document(synth.convert_model(saved, "json")) == first
            b.free()
            back.free()


def test_the_suffix_twin_is_a_numeric_model_that_routes_alike():
    js, trees, cat_max = CS.make_booster(31, 10, suffix=True)
    tw = CS.twin(js, trees, cat_max)
    assert load(tw).num_categorical_splits() == 0 and load(js).num_categorical_splits() > 0
    X = CS.rows(32, 400, cat_max, wild=False)
    CS.assert_in_twin_range(X, cat_max, np.nan)
    want, _ = CS.predict(trees, CS.base_of(js), X)
    # the twin through the super-node walk on the host (no categorical code anywhere in it)
    got, _ = synth.super_walk_cpu(tw, X, missing=float("nan"))
    assert got is not None and np.array_equal(helpers.bits(got), helpers.bits(want))
    with pytest.raises(AssertionError):
        CS.assert_in_twin_range(CS.rows(33, 400, cat_max, wild=True), cat_max, np.nan)


# ---------------------------------------------------------------- the generated code

KERNELS = ["predict_cat_tile_kernel", "predict_cat_direct_kernelILb0E", "predict_cat_direct_kernelILb1E"]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "categorical.s"
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc", "categorical.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel_body(text, name_part):
    m = re.search(r"^(_Z\w*" + re.escape(name_part) + r"\w*):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
    assert m, name_part
    return m.group(2)


@pytest.mark.parametrize("kernel", KERNELS)
def test_categorical_kernels_shape(isa, kernel):
    """No flat access, no scratch; a node is ONE 128-bit load (buffer_load_dwordx4 through the descriptor, never split
    into narrower buffer loads); the set word of a multi-word set is one global_load_dword; at most 64 VGPRs: the
    8-waves-per-SIMD step of the register file, in which the compiler's report puts all three (32, 20 and 20 VGPRs; the
    tile kernel's 102 SGPRs make it 7 waves, and its LDS tiles 5 at 27 features)."""
    body = kernel_body(isa, kernel)
    assert "flat_load" not in body and "flat_store" not in body
    assert "scratch_load" not in body and "scratch_store" not in body
    assert body.count("buffer_load_dwordx4") >= 2                                  # a root and a step at least
    assert not re.search(r"buffer_load_dword(x2|x3)?\s", body)
    assert "global_load_dword " in body
    assert "global_atomic_or" in body and "global_atomic_add" not in body           # the flag word, nothing else
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1))
    assert vgpr <= 64, vgpr
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0


def test_the_tile_kernel_reads_its_features_from_lds(isa):
    body = kernel_body(isa, "predict_cat_tile_kernel")
    assert body.count("ds_read_b32") >= 2 and "ds_write_b32" in body
    assert "s_barrier" not in body                                                  # a wave reads its own tile only
    direct = kernel_body(isa, "predict_cat_direct_kernelILb0E")
    assert "ds_read" not in direct and "ds_write" not in direct
