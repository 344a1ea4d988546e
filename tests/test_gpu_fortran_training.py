"""Every training and explaining entry point of ohx_bindings called from Fortran (tests/fortran/train_driver.F90), and
what comes back compared with the numpy restatements of include/ohxgb.h - never with the ctypes path - bit for bit:
uint32 / uint64 views of floats, array_equal of integers, grow_support.same_tree for trees.  Contributions and
interactions are held to the float64 references under the rel = 1e-5 bound of test_gpu_contribs.py and
test_gpu_interactions.py.

One process a family (cuts, refit, visits, boost, explain), one at a time.  After a driver that ended on a signal or a
time limit no further driver is started: the tests that would need one fail without starting anything.

Every scalar handed over differs from its neighbours in the argument lists, so that two dummies exchanged in a block
of ohx_bindings - which still compiles and links - cannot grow the same trees; test_exchanged_neighbours_change_the_
trees shows that on the restatement alone.  The inputs are grow_deep_support.inputs at seed 25, the first seed tried:
test_a_deep_tree_splits_at_level_8 shows that its depth-9 trees reach the histograms kept in HBM."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import contribs_support as cs
from tests import grow_deep_sampled_support as DS
from tests import grow_deep_support as D
from tests import grow_eval_support as E
from tests import grow_sampled_support as P
from tests import grow_support as G
from tests import grow_weighted_support as W
from tests import helpers
from tests import interactions_support as isup
from tests import refit_support as R
from tests import visits_support as V

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "train_driver_hip")
NAN = float("nan")
N, NHELD, NFEAT, BINS, SEED = 4097, 1000, 5, 64, 25
# no value equals a neighbour's in any of the argument lists
HYPER = dict(eta=0.3, lam=1.5, gamma=0.01, min_child_weight=2.0)
MIN_CHILD_ROWS, ROUNDS, MAX_DEPTH, DEEP_DEPTH, PATIENCE = 3, 2, 3, 9, 1
SUBSAMPLE, COLSAMPLE, DRAW_SEED = 0.5, 0.7, 5
UNVISITED, PRIOR_WEIGHT, GRID = 0, 0.25, (20, 10, 0)
UNTOUCHED = -1                   # what the driver puts into every output before a call

KINDS = ["Plain", "Eval", "Weighted", "Sampled", "Deep", "DeepSampled"]
FATAL = (124, 134, 137, 139, -6, -9, -11)


# ---- the inputs and what the header says comes back: numpy only ----

def margin(image, x):
    """The float32 margin of a JSON model over x: the base plus the leaves in tree order, one float32 add each."""
    pred = np.full(len(x), R.base_of(image), dtype=np.float32)
    for t in V.doc_trees(image):
        pred = pred + np.asarray(t["split_conditions"], dtype=np.float32)[R.walk(t, x, NAN)]
        assert pred.dtype == np.float32
    return pred


@functools.lru_cache(maxsize=None)
def inputs():
    x, y, cuts = D.inputs(N, SEED, NFEAT, BINS)
    ex, ey, _ = D.inputs(NHELD, SEED + 1, NFEAT, BINS)
    rng = np.random.default_rng(SEED + 7)
    steps = np.arange(0.0, 2.5, 0.5).astype(np.float32)
    w, ew = rng.choice(steps, N), rng.choice(steps, NHELD)
    base = R.stumps(2, nfeat=NFEAT)
    return dict(x=x, y=y, w=w, ex=ex, ey=ey, ew=ew, cuts=cuts, base=base, pred=margin(base, x), epred=margin(base, ex))


def restate(kind, **change):
    """The restatement of one boosting kind on the common inputs; `change` replaces hyper-parameters."""
    i = inputs()
    p = dict(HYPER, rounds=ROUNDS, max_depth=DEEP_DEPTH if kind.startswith("Deep") else MAX_DEPTH,
             min_child_rows=MIN_CHILD_ROWS, patience=PATIENCE, subsample=SUBSAMPLE, colsample_bytree=COLSAMPLE,
             seed=DRAW_SEED)
    p.update(change)
    tree = {k: p[k] for k in ("rounds", "max_depth", "eta", "lam", "gamma")}
    if kind == "Plain":
        return G.boost(i["pred"], i["x"], NAN, i["y"], i["cuts"], NFEAT, min_child_rows=p["min_child_rows"], **tree)
    if kind == "Eval":
        return E.boost_eval(i["pred"], i["x"], NAN, i["y"], i["cuts"], NFEAT, eval_set=(i["ex"], NAN, i["ey"]),
                            eval_pred=i["epred"], patience=p["patience"], min_child_rows=p["min_child_rows"], **tree)
    held = dict(eval_set=(i["ex"], NAN, i["ey"], i["ew"]), eval_pred=i["epred"], patience=p["patience"],
                min_child_weight=p["min_child_weight"], **tree)
    if kind == "Weighted":
        return W.boost_weighted(i["pred"], i["x"], NAN, i["y"], i["w"], i["cuts"], NFEAT, **held)
    if kind == "Deep":
        return D.boost_deep(i["pred"], i["x"], NAN, i["y"], i["w"], i["cuts"], NFEAT, **held)
    draw = dict(subsample=p["subsample"], colsample_bytree=p["colsample_bytree"], seed=p["seed"], tree0=2)
    if kind == "Sampled":
        return P.boost_sampled(i["pred"], i["x"], NAN, i["y"], i["w"], i["cuts"], NFEAT, **held, **draw)
    assert kind == "DeepSampled"
    return DS.boost_deep_sampled(i["pred"], i["x"], NAN, i["y"], i["w"], i["cuts"], NFEAT, **held, **draw)


@functools.lru_cache(maxsize=None)
def expected(kind):
    return restate(kind)


def grown(out):
    return out.get("all_trees", out["trees"])


def same_trees(a, b):
    return len(a) == len(b) and all(all(np.array_equal(s[k], t[k]) for k in G.ARRAYS) for s, t in zip(a, b))


@functools.lru_cache(maxsize=None)
def explain_image():
    """The base model with the restated trees of the Weighted call: covers on every node, depth 3."""
    kept = expected("Weighted")["trees"]
    assert len(kept) == ROUNDS
    return G.with_trees(inputs()["base"], kept)


def test_a_deep_tree_splits_at_level_8():
    """Levels from 8 on keep their histograms in HBM: the depth-9 cases must have a node that splits there."""
    for kind in ("Deep", "DeepSampled"):
        for t in grown(expected(kind)):
            per_level = D.levels(t)
            assert len(per_level) == DEEP_DEPTH + 1 and per_level[8][1] > 0, (kind, per_level)


# Neighbours of one C type in the argument lists, and the kinds whose list holds both.
PAIRS = {
    "rounds <-> max_depth": (KINDS, lambda kind: dict(rounds=DEEP_DEPTH if kind.startswith("Deep") else MAX_DEPTH,
                                                      max_depth=ROUNDS)),
    "eta <-> lambda": (KINDS, lambda kind: dict(eta=HYPER["lam"], lam=HYPER["eta"])),
    "lambda <-> gamma": (KINDS, lambda kind: dict(lam=HYPER["gamma"], gamma=HYPER["lam"])),
    "gamma <-> min_child_weight": (KINDS[2:], lambda kind: dict(gamma=HYPER["min_child_weight"],
                                                                min_child_weight=HYPER["gamma"])),
    "min_child_weight <-> subsample": (["Sampled", "DeepSampled"],
                                       lambda kind: dict(min_child_weight=SUBSAMPLE, subsample=HYPER["min_child_weight"])),
    "subsample <-> colsample_bytree": (["Sampled", "DeepSampled"],
                                       lambda kind: dict(subsample=COLSAMPLE, colsample_bytree=SUBSAMPLE)),
    "seed <-> patience": (["Sampled", "DeepSampled"], lambda kind: dict(seed=PATIENCE, patience=DRAW_SEED)),
}
# The one exchange these values cannot show: at depth 3 every node holds hundreds of rows and every best gain is far
# above 2, so gamma = 2.0 with min_child_weight = 0.01 grows the trees of gamma = 0.01 with min_child_weight = 2.0.  The
# Sampled, Deep and DeepSampled lists hold the pair at the same positions and do show it; in the Weighted blocks it is
# the dummy names of tests/test_bindings_abi_cpu.py that catch it.
INVISIBLE = [("Weighted", "gamma <-> min_child_weight")]
EXCHANGES = [(kind, what, change(kind)) for what, (kinds, change) in PAIRS.items() for kind in kinds
             if (kind, what) not in INVISIBLE]


@pytest.mark.parametrize("kind,what,change", EXCHANGES, ids=[f"{k}: {w}" for k, w, _ in EXCHANGES])
def test_exchanged_neighbours_change_the_trees(kind, what, change):
    """On the restatement alone: with two neighbouring scalars exchanged the call is refused or grows other trees."""
    values = list(change.values())
    assert values[0] != values[1]
    try:
        other = restate(kind, **change)
    except ValueError:
        return                                             # refused: a subsample of 2.0
    assert not same_trees(grown(other), grown(expected(kind))), what


# ---- the driver ----

def f32_bits(v):
    return int(np.float32(v).view(np.int32))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(DRIVER), DRIVER
    d = tmp_path_factory.mktemp("train_driver")
    i = inputs()
    for name in ("x", "y", "w", "ex", "ey", "ew"):
        np.ascontiguousarray(i[name], dtype="<f4").tofile(d / f"{name}.f32")
    (d / "base.json").write_bytes(i["base"])
    (d / "explain.json").write_bytes(explain_image())
    args = [(N, "nrow"), (NFEAT, "ncol"), (NHELD, "nheld"), (f32_bits(NAN), "missing"), (BINS, "max_bins"),
            (ROUNDS, "rounds"), (MAX_DEPTH, "max_depth"), (DEEP_DEPTH, "deep_depth"), (f32_bits(HYPER["eta"]), "eta"),
            (f32_bits(HYPER["lam"]), "lambda"), (f32_bits(HYPER["gamma"]), "gamma"), (MIN_CHILD_ROWS, "min_child_rows"),
            (f32_bits(HYPER["min_child_weight"]), "min_child_weight"), (f32_bits(SUBSAMPLE), "subsample"),
            (f32_bits(COLSAMPLE), "colsample_bytree"), (DRAW_SEED, "seed"), (PATIENCE, "patience"),
            (UNVISITED, "unvisited"), (f32_bits(PRIOR_WEIGHT), "prior_weight"), (GRID[0], "grid_im"), (GRID[1], "grid_jm"),
            (GRID[2], "grid_row0")]
    (d / "args.txt").write_text("".join(f"{v} {name}\n" for v, name in args))
    return d


_ended_badly = []
_results = {}


def run_family(workdir, family):
    """The driver's results for one family, run once: {key: int64 array}.  Fails - and starts nothing - once a driver
    has ended on a signal or a time limit."""
    if family in _results:
        return _results[family]
    if _ended_badly:
        pytest.fail(f"not started: {_ended_badly[0]}")
    try:
        r = helpers.run_driver(DRIVER, family, workdir, timeout=120)
    except subprocess.TimeoutExpired as e:
        _ended_badly.append(f"the {family} driver did not end in 120 s")
        pytest.fail(f"{_ended_badly[0]}\n{e.stdout}")
    if r.returncode in FATAL:
        _ended_badly.append(f"the {family} driver ended with status {r.returncode}")
    assert r.returncode == 0, f"train_driver {family}: status {r.returncode}\n{r.stdout}"
    lines = (workdir / f"{family}.txt").read_text().split("\n")
    out, at = {}, 0
    while at < len(lines) and lines[at]:
        key, n = lines[at].split()
        assert key not in out, key
        out[key] = np.array([int(v) for v in lines[at + 1:at + 1 + int(n)]], dtype=np.int64)
        assert len(out[key]) == int(n), key
        at += 1 + int(n)
    assert out.pop("done").tolist() == [1]
    _results[family] = out
    return out


def as_f32_bits(a):
    return np.asarray(a, dtype=np.int64).astype(np.uint32)


def one(a):
    assert len(a) == 1
    return int(a[0])


# ---- cuts ----

def test_cuts(workdir):
    got = run_family(workdir, "cuts")
    i = inputs()
    ptr, values = G.quantile_cuts(i["x"], NAN, BINS)
    assert np.array_equal(ptr, i["cuts"][0]) and len(values) > NFEAT * (BINS - 2)
    # a cap of 0 is refused with *needed set: how a caller sizes cut_values
    assert one(got["sizing_rc"]) == -1 and one(got["sizing_needed"]) == len(values) == one(got["host_needed"])
    assert np.array_equal(got["host_ptr"], ptr.astype(np.int64))
    assert np.array_equal(as_f32_bits(got["host_values"]), helpers.bits(values))
    for step in (1, 3):
        ptr, values = G.quantile_cuts(i["x"][::step], NAN, BINS)
        for matrix in ("hostmat", "devmat"):
            key = f"{matrix}_step{step}"
            assert one(got[key + "_needed"]) == len(values), key
            assert np.array_equal(got[key + "_ptr"], ptr.astype(np.int64)), key
            assert np.array_equal(as_f32_bits(got[key + "_values"]), helpers.bits(values)), key
    assert not np.array_equal(got["devmat_step3_values"], got["devmat_step1_values"])


# ---- refit ----

def test_refit(workdir):
    got = run_family(workdir, "refit")
    i = inputs()
    want = R.refit(i["base"], i["x"], NAN, i["y"], eta=HYPER["eta"], reg_lambda=HYPER["lam"], unvisited=UNVISITED)
    assert want["leaves_refit"] == 4
    images = {}
    for form in ("host", "device"):
        for how in ("loc", "null"):
            name = f"refit_{form}_{how}"
            assert one(got[name + "_leaves"]) == (want["leaves_refit"] if how == "loc" else UNTOUCHED), name
            images[name] = (workdir / f"{name}.json").read_bytes()
            value, base_weight = R.leaves_of(images[name])
            for t in range(2):
                assert np.array_equal(helpers.bits(value[t]), helpers.bits(want["value"][t])), (name, t)
                assert np.array_equal(helpers.bits(base_weight[t]), helpers.bits(want["base_weight"][t])), (name, t)
    assert len(set(images.values())) == 1                        # every form's saved model, byte for byte
    assert images["refit_host_loc"] != i["base"]


# ---- visits ----

def test_visits(workdir):
    got = run_family(workdir, "visits")
    i = inputs()
    trees = V.doc_trees(i["base"])
    offsets = np.concatenate([[0], np.cumsum([len(t["left_children"]) for t in trees])]).astype(np.int64)

    def counts_of(rows):
        return V.expected_counts(trees, np.stack([R.walk(t, rows, NAN) for t in trees], axis=1))
    train, held = counts_of(i["x"]), counts_of(i["ex"])
    for key, counts, rows in (("after_host", train, N), ("after_device", [2 * c for c in train], 2 * N),
                              ("after_reset", [0 * c for c in train], 0), ("held_out", held, NHELD)):
        assert one(got[key + "_ntree"]) == len(trees), key
        assert one(got[key + "_rows_seen"]) == rows, key
        assert np.array_equal(got[key + "_offsets"], offsets), key
        assert np.array_equal(got[key + "_counts"], np.concatenate(counts).astype(np.int64)), key
    V.check_invariants(trees, train, N)
    saved = V.doc_trees((workdir / "visits_refreshed.json").read_bytes())
    for t, (tree, c) in enumerate(zip(trees, held)):
        want = V.expected_cover(tree, c, PRIOR_WEIGHT)
        assert np.array_equal(helpers.bits(np.asarray(saved[t]["sum_hessian"], dtype=np.float32)), helpers.bits(want)), t
        assert not np.array_equal(want, np.asarray(tree["sum_hessian"], dtype=np.float32))


# ---- boost ----

def f64_bits(values):
    return np.asarray(values, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("form", ["", "Device"])
@pytest.mark.parametrize("kind", KINDS)
def test_boost(workdir, kind, form):
    got = run_family(workdir, "boost")
    name = kind + form
    want = expected(kind)
    i = inputs()
    assert one(got[name + "_nodes_added"]) == want["nodes_added"] > 0
    image = (workdir / f"boost_{name}.json").read_bytes()
    trees = G.trees_of(image)
    assert len(trees) == 2 + len(want["trees"])
    for t, old in enumerate(G.trees_of(i["base"])):               # the model's own two trees are untouched
        assert all(np.array_equal(trees[t][k], old[k]) for k in G.ARRAYS), t
    for t, tree in enumerate(want["trees"]):
        assert G.same_tree(trees[2 + t], tree) is None, (name, t, G.same_tree(trees[2 + t], tree))
    if kind != "Plain":
        run = want["rounds_run"]
        assert (one(got[name + "_rounds_run"]), one(got[name + "_best_round"])) == (run, want["best_round"])
        for which in ("train_rmse", "eval_rmse"):
            bits = got[f"{name}_{which}"]
            assert len(bits) == ROUNDS + 1
            assert np.array_equal(bits[:run + 1], f64_bits(want[which])), (name, which)
            assert np.array_equal(bits[run + 1:], f64_bits([UNTOUCHED] * (ROUNDS - run))), (name, which)
    if form:
        assert image == (workdir / f"boost_{kind}.json").read_bytes()       # the host form's, byte for byte


def test_boost_kinds_differ(workdir):
    """The kinds were handed different arguments and leave different models - but for the Eval call, whose trees are the
    plain call's by the header: both of its rounds improved the held-out error, so both were kept."""
    run_family(workdir, "boost")
    images = {kind: (workdir / f"boost_{kind}.json").read_bytes() for kind in KINDS}
    assert expected("Eval")["best_round"] == ROUNDS and images["Eval"] == images["Plain"]
    assert len(set(images.values())) == len(KINDS) - 1


# ---- explain ----

def explain_trees():
    return [{"left": t["left_children"], "right": t["right_children"], "feat": t["split_indices"],
             "cond": t["split_conditions"], "dl": t["default_left"], "cover": t["sum_hessian"]}
            for t in V.doc_trees(explain_image())]


def test_explain(workdir):
    got = run_family(workdir, "explain")
    i = inputs()
    trees, base = explain_trees(), float(R.base_of(explain_image()))
    assert len(trees) == 2 + ROUNDS
    assert one(got["contribs_len"]) == NHELD * (NFEAT + 1)
    phi = as_f32_bits(got["contribs"]).view(np.float32).reshape(NHELD, NFEAT + 1)
    worst = cs.within(phi, cs.treeshap64(trees, base, i["ex"], NAN, NFEAT))
    print(f"contributions: worst |got - ref64| / (1e-5 (1 + sum |ref|)) = {worst:.3g}")
    assert worst <= 1.0
    assert one(got["interactions_len"]) == NHELD * (NFEAT + 1) ** 2
    inter = as_f32_bits(got["interactions"]).view(np.float32).reshape(NHELD, NFEAT + 1, NFEAT + 1)
    worst = isup.within(inter, isup.interactions64(trees, base, i["ex"], NAN, NFEAT))
    print(f"interactions: worst |got - ref64| / (1e-5 (1 + sum |ref|)) = {worst:.3g}")
    assert worst <= 1.0
    assert np.abs(inter[:, :NFEAT, :NFEAT][:, ~np.eye(NFEAT, dtype=bool)]).max() > 0      # not only a diagonal
    assert one(got["predict_len"]) == NHELD and one(got["predict_same_after_set_grid"]) == 1
    assert np.array_equal(as_f32_bits(got["predict"]), helpers.bits(margin(explain_image(), i["ex"])))
    assert one(got["categorical_splits"]) == 0
