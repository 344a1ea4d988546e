"""Boosting with a held-out set on the GPU (csrc/grow_eval.hip, OHXBoosterBoostTreesEval).  Both RMSE arrays are compared
with ==, rounds_run, best_round and nodes_added as integers, and models byte for byte.

Expected values never come from the code under test: tests/grow_eval_support.py restates the call in numpy and Python
integers from the text of include/ohxgb.h.  The margins the restatement starts from are margin predicts of a FRESH booster
of the same model, as in tests/test_gpu_grow.py."""
import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import grow_eval_support as E
from tests import grow_support as G
from tests import helpers
from tests.test_gpu_grow import base_model, labels, margin_of, nfeat_of, rows, same_new_trees, held
from tests.test_grow_eval_cpu import early_stopping_case

pytestmark = pytest.mark.gpu

NAN = float("nan")
FORMATS = ("json", "ubj", "bin")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def saved(b, tmp_path):
    out = []
    for ext in FORMATS:
        path = str(tmp_path / ("m." + ext))
        b.save_model(path)
        out.append(open(path, "rb").read())
    return out


def restate(js, x, missing, y, cuts, eval_set=None, **kw):
    """eval_set: (rows, missing, labels).  Keyword names as the Python binding's."""
    pk = {"rounds": kw.get("rounds", 1), "max_depth": kw.get("max_depth", 6), "eta": kw.get("eta", 0.3),
          "lam": kw.get("reg_lambda", 1.0), "gamma": kw.get("gamma", 0.0), "min_child_rows": kw.get("min_child_rows", 1),
          "patience": kw.get("patience", 0)}
    ep = margin_of(js, eval_set[0], eval_set[1]) if eval_set is not None else None
    return E.boost_eval(margin_of(js, x, missing), x, missing, y, cuts, nfeat_of(js), eval_set=eval_set, eval_pred=ep, **pk)


def same_result(got, want, what=""):
    assert got["rounds_run"] == want["rounds_run"] and got["best_round"] == want["best_round"], (what, got, want["rounds_run"], want["best_round"])
    assert got["nodes_added"] == want["nodes_added"], (what, got["nodes_added"], want["nodes_added"])
    assert got["train_rmse"].tolist() == want["train_rmse"], (what, got["train_rmse"], want["train_rmse"])
    if want["eval_rmse"] is None:
        assert got["eval_rmse"] is None, what
    else:
        assert got["eval_rmse"].tolist() == want["eval_rmse"], (what, got["eval_rmse"], want["eval_rmse"])


def check(tmp_path, js, x, missing, y, cuts, ev, what="", grid=None, egrid=None, **kw):
    """One host-form call on a fresh booster against the restatement.  ev: (rows, missing, labels) or None.
    -> (the restatement, the result, the booster)."""
    want = restate(js, x, missing, y, cuts, ev, **kw)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=missing)
    if grid is not None:
        d.set_grid(*grid)
    ed = None
    if ev is not None:
        ed = capi.DMatrix(ev[0], missing=ev[1])
        if egrid is not None:
            ed.set_grid(*egrid)
    got = b.boost_trees_eval(d, y, cuts, eval_set=(ed, ev[2]) if ev is not None else None, **kw)
    same_result(got, want, what)
    nold = len(G.trees_of(synth.convert_model(js, "json")))
    same_new_trees(held(b, tmp_path)[0], want["trees"], nold, what)
    d.free()
    if ed is not None:
        ed.free()
    return want, got, b


def case(nfeat, ntrain, neval, missing=NAN, emissing=NAN, ecols=None, seed=0, ntree=3):
    """A model, training rows and labels, held-out rows (ecols columns) and labels, cuts."""
    js = base_model(nfeat, ntree)
    x = rows(seed + ntrain * 7 + nfeat, ntrain, nfeat, missing)
    y = labels(seed + ntrain, x, margin_of(js, x, missing))
    ex = rows(seed + neval * 11 + nfeat + 1, neval, nfeat, emissing)
    ey = labels(seed + neval + 1, ex, margin_of(js, ex, emissing))
    if ecols is not None:
        ex = np.ascontiguousarray(ex[:, :ecols])
    return js, x, y, ex, ey, capi.quantile_cuts(x, missing, 64)


# ---- patience = 0 keeps all trees ----

@pytest.mark.parametrize("nfeat,max_depth,rounds", [(1, 1, 5), (3, 6, 1), (27, 8, 5), (3, 8, 1), (27, 1, 1)])
def test_patience_0_leaves_what_the_plain_call_leaves(torch_cuda, tmp_path, nfeat, max_depth, rounds):
    js, x, y, ex, ey, cuts = case(nfeat, 1000, 300, missing=-999.0)
    kw = dict(rounds=rounds, max_depth=max_depth, eta=0.5)
    twin = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=-999.0)
    ed = capi.DMatrix(ex, missing=NAN)
    n_plain = twin.boost_trees(d, y, cuts, **kw)
    want_bytes = saved(twin, tmp_path)
    for what, ev in (("held-out set", (ed, ey)), ("no held-out set", None), ("the training set held out", (d, y))):
        b = capi.Booster(model_buffer=js)
        got = b.boost_trees_eval(d, y, cuts, eval_set=ev, patience=0, **kw)
        assert got["nodes_added"] == n_plain and got["rounds_run"] == rounds, what
        assert saved(b, tmp_path) == want_bytes, what
        b.free()
    for m in (d, ed):
        m.free()
    twin.free()


# ---- both RMSE arrays equal the restatement's ----

@pytest.mark.parametrize("neval", (1, 63, 64, 65, 4097))
@pytest.mark.parametrize("ntrain", (64, 4097))
def test_rmse_equals_the_restatement(torch_cuda, tmp_path, ntrain, neval):
    emissing = -999.0 if (ntrain + neval) % 2 else NAN
    js, x, y, ex, ey, cuts = case(3, ntrain, neval, missing=NAN, emissing=emissing)
    want, got, b = check(tmp_path, js, x, NAN, y, cuts, (ex, emissing, ey), f"{ntrain} / {neval} rows", rounds=3, max_depth=6, eta=0.5)
    assert want["train_rmse"][-1] < want["train_rmse"][0]
    if neval >= 4097:
        assert np.isnan(ex).any() and (emissing != emissing or (ex == emissing).any())
    b.free()


def test_a_held_out_matrix_with_fewer_columns_than_features(torch_cuda, tmp_path):
    js, x, y, ex, ey, cuts = case(5, 1000, 777, ecols=3)
    want, got, b = check(tmp_path, js, x, NAN, y, cuts, (ex, NAN, ey), "three columns of five", rounds=3, max_depth=5, eta=0.5)
    used = np.concatenate([t["feature"][t["left"] >= 0] for t in want["trees"]])
    assert (used >= 3).any(), "a split on a column the held-out matrix lacks"
    b.free()


def test_the_form_the_stream_the_order_of_the_rows_and_the_grid_change_no_bit(torch_cuda, tmp_path):
    torch = torch_cuda
    js, x, y, ex, ey, cuts = case(27, 1200, 1300, missing=-999.0, emissing=-999.0)
    kw = dict(rounds=3, max_depth=5, eta=0.5, patience=2)
    want = restate(js, x, -999.0, y, cuts, (ex, -999.0, ey), **kw)
    perm = np.random.default_rng(1).permutation(len(ex))
    exp, eyp = np.ascontiguousarray(ex[perm]), np.ascontiguousarray(ey[perm])
    for what, erows, elab, egrid, device in (("plain", ex, ey, None, False), ("held-out rows permuted", exp, eyp, None, False),
                                             ("a grid said on the held-out matrix", ex, ey, (13, 10, 0), False),
                                             ("device form on a stream", ex, ey, None, True),
                                             ("device form, permuted, grid said", exp, eyp, (13, 10, 0), True)):
        b = capi.Booster(model_buffer=js)
        if device:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                tx, ty = torch.from_numpy(x).to("cuda"), torch.from_numpy(y).to("cuda")
                tex, tey = torch.from_numpy(erows).to("cuda"), torch.from_numpy(elab).to("cuda")
            s.synchronize()
            d = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=len(x), ncol=27, missing=-999.0)
            ed = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=len(erows), ncol=27, missing=-999.0)
        else:
            d = capi.DMatrix(x, missing=-999.0)
            ed = capi.DMatrix(erows, missing=-999.0)
        if egrid is not None:
            ed.set_grid(*egrid)
        if device:
            got = b.boost_trees_eval_device(d, ty.data_ptr(), len(y), cuts, eval_set=(ed, tey.data_ptr(), len(elab)),
                                            stream=s.cuda_stream, **kw)
        else:
            got = b.boost_trees_eval(d, y, cuts, eval_set=(ed, elab), **kw)
        same_result(got, want, what)
        same_new_trees(held(b, tmp_path)[0], want["trees"], 3, what)
        for m in (d, ed):
            m.free()
        b.free()


def test_a_device_held_out_matrix_with_a_host_training_matrix(torch_cuda, tmp_path):
    """Both matrix forms in one host-form call."""
    torch = torch_cuda
    js, x, y, ex, ey, cuts = case(3, 500, 600)
    kw = dict(rounds=2, max_depth=4)
    want = restate(js, x, NAN, y, cuts, (ex, NAN, ey), **kw)
    tex = torch.from_numpy(ex).cuda()
    torch.cuda.synchronize()
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=NAN)
    ed = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=len(ex), ncol=3, missing=NAN)
    same_result(b.boost_trees_eval(d, y, cuts, eval_set=(ed, ey), **kw), want)
    for m in (d, ed):
        m.free()
    b.free()


# ---- the held-out set is the training set ----

def test_the_training_set_held_out_gives_the_same_sums_by_the_walk(torch_cuda, tmp_path):
    """The walk kernel against the partition path: same handle, same labels."""
    js, x, y, _, _, cuts = case(3, 4097, 1, missing=-999.0)
    kw = dict(rounds=4, max_depth=8, eta=0.5)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=-999.0)
    got = b.boost_trees_eval(d, y, cuts, eval_set=(d, y), **kw)
    assert got["eval_rmse"].tolist() == got["train_rmse"].tolist()
    same_result(got, restate(js, x, -999.0, y, cuts, (x, -999.0, y), **kw))
    assert got["best_round"] == 4 and got["train_rmse"][4] < got["train_rmse"][0]
    d.free()
    b.free()


# ---- past the launch cap ----

def test_more_held_out_rows_than_two_trips_of_the_grid_stride_loop(torch_cuda, tmp_path):
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = synth.grow_eval_plan(1 << 30, cus)["blocks"]
    neval = 2 * 256 * blocks + 1
    assert synth.grow_eval_plan(neval, cus)["blocks"] == blocks
    js = base_model(2, 1)
    rng = np.random.default_rng(9)
    def make(n):
        x = np.empty((n, 2), dtype=np.float32)
        x[:, 0] = rng.integers(0, 10, n)
        x[:, 1] = rng.integers(0, 2, n)
        x[rng.random(n) < 0.01, 0] = np.nan
        y = (margin_of(js, x, NAN) + np.nan_to_num(x[:, 0]) * 0.1 - x[:, 1] + rng.normal(0, 0.1, n)).astype(np.float32)
        return x, y
    x, y = make(5000)
    ex, ey = make(neval)
    cuts = capi.quantile_cuts(x, NAN)
    want, got, b = check(tmp_path, js, x, NAN, y, cuts, (ex, NAN, ey), "past the launch cap", rounds=2, max_depth=2, eta=0.5)
    assert want["eval_sums"][2] < want["eval_sums"][1] < want["eval_sums"][0]
    b.free()


# ---- the product's edge ----

def test_the_edge_of_the_product_and_eval_labels_out_of_range(torch_cuda, tmp_path):
    """A model of 0 trees and base 0; gamma above every gain keeps each new tree a root leaf; the training labels are 0,
    so that leaf is -0.0 and the held-out margin stays 0: the residuals are the negated eval labels."""
    js = G.empty_model(2, base=0.0)
    x = rows(1, 64, 2, NAN)
    y = np.zeros(64, np.float32)
    cuts = capi.quantile_cuts(x, NAN)
    ex = np.zeros((2, 2), np.float32)
    edge = np.float32(256.0 - 2.0 ** -16)
    assert np.nextafter(edge, np.float32(1000)) == np.float32(256.0)
    kw = dict(rounds=2, gamma=1e9)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=NAN)
    ed = capi.DMatrix(ex, missing=NAN)
    before = saved(b, tmp_path)
    ey = np.array([edge, -edge], np.float32)
    want = restate(js, x, NAN, y, cuts, (ex, NAN, ey), **kw)
    q = (1 << 32) - 256
    assert want["eval_sums"] == [2 * q * q] * 3 and 2 * q * q > 1 << 64
    same_result(b.boost_trees_eval(d, y, cuts, eval_set=(ed, ey), **kw), want, "the edge")
    b.load_model_buffer(js)
    for bad in (np.float32(256.0), np.float32(-256.0), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)):
        eb = np.array([0.5, bad], np.float32)
        with pytest.raises(ValueError, match="eval label"):
            restate(js, x, NAN, y, cuts, (ex, NAN, eb), **kw)
        with pytest.raises(capi.OhxError, match="eval label") as err:
            b.boost_trees_eval(d, y, cuts, eval_set=(ed, eb), **kw)
        assert "unchanged" in str(err.value)
        assert saved(b, tmp_path) == before, bad
        # a valid call follows
        same_result(b.boost_trees_eval(d, y, cuts, eval_set=(ed, ey), **kw), want, f"after {bad}")
        b.load_model_buffer(js)
    for m in (d, ed):
        m.free()
    b.free()


# ---- early stopping ----

def test_early_stopping_with_the_best_round_strictly_inside(torch_cuda, tmp_path):
    xt, yt, xe, ye, cuts = early_stopping_case()
    js = G.empty_model(3, base=0.0)
    kw = dict(rounds=20, max_depth=6, eta=0.5, reg_lambda=1.0, patience=3)
    want = restate(js, xt, NAN, yt, cuts, (xe, NAN, ye), **kw)
    assert 0 < want["best_round"] < want["rounds_run"] < 20
    assert (want["best_round"], want["rounds_run"]) == (4, 7)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(xt, missing=NAN)
    ed = capi.DMatrix(xe, missing=NAN)
    got = b.boost_trees_eval(d, yt, cuts, eval_set=(ed, ye), **kw)
    same_result(got, want, "early stopping")
    assert len(got["train_rmse"]) == 8 and len(got["eval_rmse"]) == 8
    # the saved model is what the plain call leaves after `best` rounds
    twin = capi.Booster(model_buffer=js)
    plain = dict(kw, rounds=want["best_round"])
    del plain["patience"]
    assert twin.boost_trees(d, yt, cuts, **plain) == got["nodes_added"]
    assert saved(b, tmp_path) == saved(twin, tmp_path)
    # the truncated forest predicts by every kernel, and contributions work
    for kernel, split in (("auto", "auto"), ("wide", "auto"), ("ring", "off")):
        b.set_param("ohx_kernel", kernel)
        b.set_param("ohx_tree_split", split)
        assert np.array_equal(helpers.bits(b.predict(ed, option_mask=1)), helpers.bits(want["eval_pred"])), kernel
        assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(want["pred"])), kernel
    dx = capi.DMatrix(xe[:96], missing=NAN)
    m = b.predict(dx, option_mask=1).astype(np.float64)
    phi = b.predict_contribs(dx).astype(np.float64)
    assert np.all(np.abs(phi.sum(axis=1) - m) <= 1e-5 * (1.0 + np.abs(phi).sum(axis=1)))
    for mtx in (d, ed, dx):
        mtx.free()
    for bb in (b, twin):
        bb.free()


def test_best_round_0_appends_nothing(torch_cuda, tmp_path):
    """Held-out labels that are the negated training target: every tree hurts."""
    js = base_model(3)
    x = rows(21, 1000, 3, NAN)
    margin = margin_of(js, x, NAN)
    target = labels(21, x, np.zeros(1000, np.float32))
    y = (margin + target).astype(np.float32)
    ey = (margin - target).astype(np.float32)
    cuts = capi.quantile_cuts(x, NAN, 64)
    kw = dict(rounds=6, max_depth=4, eta=0.5, patience=2)
    want = restate(js, x, NAN, y, cuts, (x, NAN, ey), **kw)
    assert (want["best_round"], want["rounds_run"], want["nodes_added"]) == (0, 2, 0)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=NAN)
    before = saved(b, tmp_path)
    m0 = b.predict(d, option_mask=1).copy()            # uploaded before the call
    same_result(b.boost_trees_eval(d, y, cuts, eval_set=(d, ey), **kw), want, "best == 0")
    assert saved(b, tmp_path) == before
    assert np.array_equal(helpers.bits(b.predict(d, option_mask=1)), helpers.bits(m0))
    # and a valid call that keeps trees follows
    same_result(b.boost_trees_eval(d, y, cuts, eval_set=(d, y), **kw), restate(js, x, NAN, y, cuts, (x, NAN, y), **kw))
    d.free()
    b.free()


def test_no_held_out_set_writes_the_training_rmse_alone(torch_cuda, tmp_path):
    js, x, y, _, _, cuts = case(3, 777, 1)
    want, got, b = check(tmp_path, js, x, NAN, y, cuts, None, "no held-out set", rounds=3, max_depth=4)
    assert got["eval_rmse"] is None and got["best_round"] == got["rounds_run"] == 3
    # the held-out array is untouched
    d = capi.DMatrix(x, missing=NAN)
    ptr, vals = b._cuts(cuts)
    import ctypes as C
    train, heldout = np.full(4, -7.0), np.full(4, -7.0)
    r, k, n = C.c_int32(), C.c_int32(), C.c_uint64()
    rc = b.lib.OHXBoosterBoostTreesEval(b.handle, d.handle, y.ctypes.data, y.size, None, None, 0, ptr.ctypes.data,
                                        vals.ctypes.data, 2, 4, 0.3, 1.0, 0.0, 1, 0, train.ctypes.data, heldout.ctypes.data,
                                        C.byref(r), C.byref(k), C.byref(n))
    assert rc == 0 and np.all(heldout == -7.0) and np.all(train[:3] != -7.0) and train[3] == -7.0, "entries past rounds_run"
    d.free()
    b.free()


# ---- refusals on the GPU ----

def test_refusals_leave_the_model_unchanged_and_a_valid_call_follows(torch_cuda, tmp_path):
    torch = torch_cuda
    js, x, y, ex, ey, cuts = case(3, 1000, 300)
    kw = dict(rounds=2, max_depth=3, patience=1)
    want = restate(js, x, NAN, y, cuts, (ex, NAN, ey), **kw)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=NAN)
    ed = capi.DMatrix(ex, missing=NAN)
    before = saved(b, tmp_path)

    def valid(what):
        assert saved(b, tmp_path) == before, what
        same_result(b.boost_trees_eval(d, y, cuts, eval_set=(ed, ey), **kw), want, what)
        b.load_model_buffer(js)

    stale = capi.DMatrix(ex, missing=NAN)
    stale_handle = stale.handle
    stale.free()
    class Stale:
        handle = stale_handle
    with pytest.raises(capi.OhxError, match="held-out DMatrix handle is invalid"):
        b.boost_trees_eval(d, y, cuts, eval_set=(Stale, ey), **kw)
    valid("a stale held-out handle")
    for nl in (len(ey) - 1, len(ey) + 1):
        with pytest.raises(capi.OhxError, match=f"{nl} eval labels for {len(ey)} held-out rows"):
            b.boost_trees_eval(d, y, cuts, eval_set=(ed, np.zeros(nl, np.float32)), **kw)
    valid("eval labels of another size")
    wide = capi.DMatrix(np.zeros((4, 4), dtype=np.float32), missing=NAN)
    with pytest.raises(capi.OhxError, match="Number of columns"):
        b.boost_trees_eval(d, y, cuts, eval_set=(wide, np.zeros(4, np.float32)), **kw)
    wide.free()
    valid("more columns than features")
    # a training label out of range is still "label", not "eval label"
    yb = y.copy()
    yb[5] = np.nan
    with pytest.raises(capi.OhxError, match="label") as err:
        b.boost_trees_eval(d, yb, cuts, eval_set=(ed, ey), **kw)
    assert "eval label" not in str(err.value)
    valid("a NaN training label")
    # a stream that is being captured
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    tex, tey = torch.from_numpy(ex).cuda(), torch.from_numpy(ey).cuda()
    dd = capi.DMatrix(device_ptr=tx.data_ptr(), nrow=len(x), ncol=3, missing=NAN)
    de = capi.DMatrix(device_ptr=tex.data_ptr(), nrow=len(ex), ncol=3, missing=NAN)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(capi.OhxError, match="stream capture"):
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            b.boost_trees_eval_device(dd, ty.data_ptr(), len(y), cuts, eval_set=(de, tey.data_ptr(), len(ey)),
                                      stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert saved(b, tmp_path) == before, "a captured stream"
    with torch.cuda.stream(s):
        got = b.boost_trees_eval_device(dd, ty.data_ptr(), len(y), cuts, eval_set=(de, tey.data_ptr(), len(ey)),
                                        stream=s.cuda_stream, **kw)
    same_result(got, want, "after the capture")
    for m in (d, ed, dd, de):
        m.free()
    b.free()


# ---- two calls in a row ----

def test_a_second_call_continues_from_the_longer_forest(torch_cuda, tmp_path):
    js, x, y, ex, ey, cuts = case(3, 1000, 500)
    kw = dict(rounds=3, max_depth=4, eta=0.5, patience=0)
    b = capi.Booster(model_buffer=js)
    d = capi.DMatrix(x, missing=NAN)
    ed = capi.DMatrix(ex, missing=NAN)
    first = restate(js, x, NAN, y, cuts, (ex, NAN, ey), **kw)
    same_result(b.boost_trees_eval(d, y, cuts, eval_set=(ed, ey), **kw), first, "first")
    _, image = held(b, tmp_path)
    second = restate(image, x, NAN, y, cuts, (ex, NAN, ey), **kw)
    got = b.boost_trees_eval(d, y, cuts, eval_set=(ed, ey), **kw)
    same_result(got, second, "second")
    assert second["train_rmse"][0] == first["train_rmse"][3] and second["eval_rmse"][0] == first["eval_rmse"][3]
    same_new_trees(held(b, tmp_path)[0], first["trees"] + second["trees"], 3, "both calls")
    for m in (d, ed):
        m.free()
    b.free()
