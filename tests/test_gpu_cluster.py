"""The three pieces of the predict path that only decide which rows share a wave, on the GPU, against
tests/cluster_support.py: the clustering keys and their `agree` words (cluster_keys_kernel), the sort of the (key, row)
pairs (sort_pairs_u32) and the level search (detect_period_kernel, and what OHXDMatrixInferGrid adopts) - through the
probes of csrc/probe_gpu.hip, which run the product's own objects on the test's buffers - and the wiring of all of it in
the product, read from OHX_DEBUG in a child process.  Integers throughout: everything is compared with ==."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import booster_shapes as S
from tests import cluster_support as K
from tests import helpers
from tests.test_adversarial_boosters_cpu import MISSING

pytestmark = pytest.mark.gpu

PATTERN = np.uint32(0xA5A5A5A5)
GUARD = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _dev(torch, a):
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)        # (the shared rows are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _pattern(torch, n):
    return _dev(torch, np.full(n, PATTERN, dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def _records(name, pack):
    """emit_super's records and heads of booster(name) in HBM, uploaded as they are."""
    import torch
    rec = synth.super_records_cpu(K.booster(name)[0], pack)
    assert rec is not None
    return _dev(torch, rec["nodes"]), _dev(torch, rec["heads"])


def _tall(name, missing, nrow, seed=3):
    """nrow rows for booster(name): its 3000, then shuffled copies of them."""
    rows = K.rows(name, missing)
    if nrow <= len(rows):
        return np.ascontiguousarray(rows[:nrow])
    rng = np.random.default_rng(seed)
    parts = [rows] + [rows[rng.permutation(len(rows))] for _ in range((nrow - 1) // len(rows))]
    return np.ascontiguousarray(np.concatenate(parts)[:nrow])


def _check_keys(torch, name, rows, ncol, missing, shape, pack=2, num_cus=256):
    """One launch of the key kernel against the reference: every key, every row number, the nine words, and nothing
    written beside them."""
    _, trees, heads = K.booster(name)
    ntrees, nsteps, zorder = shape
    rows = np.ascontiguousarray(rows[:, :ncol])
    nrow = len(rows)
    nodes, dheads = _records(name, pack)
    keys, vals = _pattern(torch, nrow + GUARD), _pattern(torch, nrow + GUARD)
    words = np.full(9 + 7, PATTERN, dtype=np.uint32)
    words[:9] = 0                                   # ClusterArgs::agree: zero before
    agree = _dev(torch, words)
    synth.probe_cluster_keys(nodes, dheads, S.NFEAT, _dev(torch, rows), ncol, missing, ntrees, nsteps, zorder, keys, vals,
                             agree, num_cus, nrow=nrow)
    torch.cuda.synchronize()
    keys, vals, agree = _host_u32(keys), _host_u32(vals), _host_u32(agree)
    what = (name, ncol, missing, shape, pack, num_cus, nrow)
    assert (keys[nrow:] == PATTERN).all() and (vals[nrow:] == PATTERN).all() and (agree[9:] == PATTERN).all(), what
    want = K.keys(trees, heads, rows, ncol, missing, ntrees, nsteps, zorder)
    bad = np.flatnonzero(keys[:nrow] != want)
    assert bad.size == 0, (what, bad.size, bad[:8], keys[bad[:8]], want[bad[:8]])
    assert np.array_equal(vals[:nrow], np.arange(nrow, dtype=np.uint32)), what
    assert int(agree[1:9].sum()) == nrow, (what, agree[:9])            # no row counted twice, none left out
    assert np.array_equal(agree[:9], K.agree(K.leads(want, ntrees, nsteps, zorder), nrow)), (what, agree[:9])
    return want


def _boosters_for(ntrees):
    # the big adversarial booster and the benchmark's shape, and the small booster whose every tree is in the key
    return [n for n in (135, "synth", {1: 1, 2: 2, 3: 3, 4: 5}[ntrees], 3) if n == "synth" or n >= ntrees]


# ---- the keys and the nine words ----

@pytest.mark.parametrize("shape", K.KEY_SHAPES, ids=lambda s: "trees%d_steps%d_z%d" % s)
def test_keys_of_every_shape_booster_and_missing_marker(torch_cuda, shape):
    """3000 rows (47 tiles, the last one of 56 rows), half of them on thresholds; both infinities and NaN among them
    where the marker is an infinity.  Booster 3 with -inf as the marker is the case that found the kernel reading
    fillers (docs/30_cluster_and_level_search_tests.md)."""
    for name in dict.fromkeys(_boosters_for(shape[0])):
        for missing in MISSING:
            _check_keys(torch_cuda, name, K.rows(name, missing), S.NFEAT, missing, shape)


@pytest.mark.parametrize("nrow", (1, 63, 64, 65, 255, 256, 257, 4097))
def test_keys_at_every_row_count(torch_cuda, nrow):
    """One row; a wave less one, exactly, and one more; a block of four waves less one row, exactly, and one more."""
    for name in (135, "synth"):
        for shape in ((2, 7, 0), (2, 7, 1), (4, 3, 1)):
            for missing in (-999.0, float("nan")):
                _check_keys(torch_cuda, name, _tall(name, missing, nrow), S.NFEAT, missing, shape)


@pytest.mark.parametrize("ncol", (27, 26, 20, 16, 3, 2, 1))
def test_keys_at_every_column_count(torch_cuda, ncol):
    """The coalesced loader steps (row, feature) differently for column counts that divide 64 and those that do not;
    the columns the matrix does not have are missing."""
    for name in (135, "synth"):
        for shape in ((2, 7, 0), (3, 4, 1), (4, 3, 0)):
            for missing in (-999.0, float("inf")):
                for nrow in (3000, 65):
                    _check_keys(torch_cuda, name, K.rows(name, missing)[:nrow], ncol, missing, shape)


@pytest.mark.parametrize("pack", synth.SUPER_PACKS)
def test_keys_do_not_depend_on_the_placement_of_the_records(torch_cuda, pack):
    for name in (135, "synth", 5):
        for shape in ((2, 7, 0), (4, 3, 1)):
            _check_keys(torch_cuda, name, K.rows(name, float("-inf")), S.NFEAT, float("-inf"), shape, pack=pack)


@pytest.mark.parametrize("name", (135, "synth", 3))
def test_a_wave_that_takes_many_tiles_in_turn(torch_cuda, name):
    """A grid sized for one CU: every wave runs the tile loop several times over the same LDS; a tile read before it
    was rewritten, or a row counted twice, shows in the keys and in the nine words."""
    for shape, missing in (((2, 7, 0), -999.0), ((4, 3, 1) if name != 3 else (3, 4, 1), float("-inf"))):
        _check_keys(torch_cuda, name, _tall(name, missing, 20_000), S.NFEAT, missing, shape, num_cus=1)
        _check_keys(torch_cuda, name, _tall(name, missing, 20_000)[:, :20], 20, missing, shape, num_cus=1)


def test_the_launcher_refuses_and_touches_nothing(torch_cuda):
    torch = torch_cuda
    rows = K.rows(3, -999.0)[:200]
    nodes, dheads = _records(3, 2)
    for ntrees, nsteps, ncol in ((0, 7, 27), (5, 1, 27), (4, 3, 27),          # none; too many; more than the booster's 3
                                 (2, 8, 27), (1, 16, 27), (3, 5, 27),          # 34, 33, 33 key bits
                                 (2, 7, 28)):                                  # more columns than features
        keys, vals, agree = _pattern(torch, 200), _pattern(torch, 200), _pattern(torch, 9)
        wide = np.ascontiguousarray(np.resize(rows, (200, ncol)))
        with pytest.raises(capi.OhxError, match="launch_cluster_keys: hipErrorInvalidValue"):
            synth.probe_cluster_keys(nodes, dheads, S.NFEAT, _dev(torch, wide), ncol, -999.0, ntrees, nsteps, 0, keys, vals,
                                     agree, 256, nrow=200)
        torch.cuda.synchronize()
        for t in (keys, vals, agree):
            assert (_host_u32(t) == PATTERN).all(), (ntrees, nsteps, ncol)
    # and the same call with what it accepts goes through
    _check_keys(torch, 3, rows, S.NFEAT, -999.0, (3, 4, 0))


# ---- the sort ----

def _sort_inputs(torch, n, rng):
    """Four key arrays of n words: the kernel's own (the default key of the benchmark-shaped booster), all equal,
    two values, random words."""
    name, missing = "synth", -999.0
    rows = _tall(name, missing, n, seed=n)
    own = _check_keys(torch, name, rows, S.NFEAT, missing, (2, 7, 0)) if n <= 4097 else None
    if own is None:                                     # (checked above at the smaller sizes: here only made)
        _, trees, heads = K.booster(name)
        nodes, dheads = _records(name, 2)
        keys, vals, agree = _pattern(torch, n), _pattern(torch, n), _dev(torch, np.zeros(9, dtype=np.uint32))
        synth.probe_cluster_keys(nodes, dheads, S.NFEAT, _dev(torch, rows), S.NFEAT, missing, 2, 7, 0, keys, vals, agree, 256)
        torch.cuda.synchronize()
        own = _host_u32(keys).copy()
    return {"own": own, "equal": np.full(n, 0x5A5A5A5A, dtype=np.uint32), "top": None,
            "random": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}


@pytest.mark.parametrize("n", (1, 2, 64, 65, 4097, 100_003))
def test_sort_pairs_orders_by_the_low_key_bits_alone(torch_cuda, n):
    """rocPRIM documents radix_sort_pairs as stable (rocprim/device/device_radix_sort.hpp: "preserves the relative
    ordering of equivalent keys"), so the permutation is np.argsort(kind="stable") of the masked keys, word for word."""
    torch = torch_cuda
    rng = np.random.default_rng(n)
    inputs = _sort_inputs(torch, n, rng)
    for key_bits in (1, 3, 27, 31, 32):
        mask = np.uint32((1 << key_bits) - 1)
        # only the top bit of the sorted range differs; above it garbage that must not count
        garbage = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & ~mask
        inputs["top"] = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(key_bits - 1)).astype(np.uint32) | garbage
        for kind, key in inputs.items():
            keys = [_dev(torch, key), _pattern(torch, n + GUARD)]
            vals = [_dev(torch, np.arange(n, dtype=np.uint32)), _pattern(torch, n + GUARD)]
            which, temp_bytes = synth.probe_sort_pairs(keys[0], keys[1], vals[0], vals[1], n, key_bits)
            what = (n, key_bits, kind, which, temp_bytes)
            assert which in (0, 1) and temp_bytes > 0, what
            got = _host_u32(vals[which])[:n]
            assert (_host_u32(vals[1])[n:] == PATTERN).all() and (_host_u32(keys[1])[n:] == PATTERN).all(), what
            assert np.array_equal(np.sort(got), np.arange(n, dtype=np.uint32)), what         # a permutation of 0 .. n-1
            masked = (key & mask)[got]
            assert (masked[1:] >= masked[:-1]).all(), what
            assert np.array_equal(got, np.argsort(key & mask, kind="stable").astype(np.uint32)), what


# ---- the level search ----

def _levels(nlev, ncell, ncol, periodic, seed=0):
    """nlev levels of ncell rows, ncol columns of random values, the `periodic` columns the same in every level."""
    rng = np.random.default_rng(seed)
    data = rng.random((nlev * ncell, ncol), dtype=np.float32) + np.float32(1.0)
    for c in periodic:
        data[:, c] = np.tile(data[:ncell, c], nlev)
    return data


def _nan(payload):
    return np.array([0x7FC00000 | payload], dtype=np.uint32).view(np.float32)[0]


def _signed_zero_levels():
    d = _levels(2, 4096, 27, ())
    d[:4096, 0], d[4096:, 0] = 0.0, -0.0
    return d


def _nan_levels(a, b):
    d = _levels(2, 4096, 27, ())
    d[:4096, 0], d[4096:, 0] = _nan(a), _nan(b)
    return d


def _defect(data, row, col=0):
    data = data.copy()
    data[row, col] = np.float32(7.0)
    return data


def _shuffled(data, seed=1):
    return data[np.random.default_rng(seed).permutation(len(data))]


# name -> (matrix, {k: word} expected of column 0's row where the table of the issue names it, adopted period)
LEVEL_CASES = {
    "2_levels_of_4096": lambda: (_levels(2, 4096, 27, (0,)), {2: 0}, 4096),
    "3_levels_of_4099": lambda: (_levels(3, 4099, 27, (0,)), {3: 0, 2: 2}, 4099),
    "12_levels_of_4096": lambda: (_levels(12, 4096, 27, (0,)),
                                  {12: 0, 6: 0, 4: 0, 3: 0, 2: 0, 8: 1, 5: 2, 7: 2, 9: 2, 10: 2, 11: 2}, 4096),
    "defect_in_row_0": lambda: (_defect(_levels(12, 4096, 27, (0,)), 0), {12: 1, 6: 1, 4: 1, 3: 1, 2: 1, 8: 1}, 0),
    "defect_in_the_last_row": lambda: (_defect(_levels(12, 4096, 27, (0,)), 12 * 4096 - 1), {12: 1, 6: 1, 4: 1, 3: 1, 2: 1, 8: 1}, 0),
    # 6 levels of 2048: every candidate (k = 3, 2) divides and holds - until the defect
    "defect_in_row_0_every_k_holds": lambda: (_defect(_levels(6, 2048, 27, (0,)), 0), {3: 1, 2: 1}, 0),
    "defect_in_the_last_row_every_k_holds": lambda: (_defect(_levels(6, 2048, 27, (0,)), 6 * 2048 - 1), {3: 1, 2: 1}, 0),
    "minus_zero_against_plus_zero": lambda: (_signed_zero_levels(), {2: 1}, 0),
    "nans_of_equal_payload": lambda: (_nan_levels(5, 5), {2: 0}, 4096),
    "nans_of_different_payload": lambda: (_nan_levels(5, 6), {2: 1}, 0),
    "periodic_only_in_the_last_column": lambda: (_levels(12, 4096, 27, (26,)), {12: 1, 8: 1, 2: 1, 5: 2}, 4096),
    "periodic_only_in_column_21": lambda: (_levels(3, 4099, 27, (21,)), {3: 1, 2: 2}, 4099),
    "periodic_only_in_column_22": lambda: (_levels(12, 4096, 27, (22,)), {12: 1, 8: 1}, 4096),
    "20_columns": lambda: (_levels(12, 4096, 20, (19,)), {12: 1}, 4096),
    "20_columns_nothing_periodic": lambda: (_levels(12, 4096, 20, ()), {12: 1, 5: 2}, 0),
    "1_column": lambda: (_levels(12, 4096, 1, (0,)), {12: 0, 8: 1, 5: 2}, 4096),
    "1_column_not_periodic": lambda: (_levels(3, 4099, 1, ()), {3: 1, 2: 2}, 0),
    "shuffled_rows": lambda: (_shuffled(_levels(12, 4096, 27, (0, 21, 22, 26))), {12: 1, 6: 1, 4: 1, 3: 1, 2: 1, 8: 1, 5: 2}, 0),
}


@pytest.mark.parametrize("case", sorted(LEVEL_CASES))
def test_level_search_verdicts_and_the_adopted_size(torch_cuda, case):
    torch = torch_cuda
    data, column0, adopted = LEVEL_CASES[case]()
    nrow, ncol = data.shape
    kmax = min(1024, nrow // 4096)                             # csrc/capi.cpp level_candidates
    cols = [0, ncol - 1, 21, 22]                               # ... and level_columns
    want = K.period_verdict(data, cols, kmax)
    for k, word in column0.items():
        assert want[0, kmax - k] == word, (case, k)            # the reference says what the issue's table says
    if ncol <= 21:
        assert (want[2:] == 2).all()
    if ncol == 1:
        assert np.array_equal(want[0], want[1])
    ddata = _dev(torch, data)
    words = np.full(4 * (kmax - 1) + GUARD, PATTERN, dtype=np.uint32)
    words[:4 * (kmax - 1)] = 0                                 # zero before (csrc/kernels.hpp)
    verdict = _dev(torch, words)
    synth.probe_detect_period(ddata, nrow, ncol, cols, kmax, verdict)
    torch.cuda.synchronize()
    got = _host_u32(verdict)
    assert (got[4 * (kmax - 1):] == PATTERN).all()
    got = got[:4 * (kmax - 1)].reshape(4, kmax - 1)
    assert np.array_equal(got, want), (case, got, want)
    # what the host makes of the words, and what the product adopts for the same matrix
    assert synth.pick_level_period(got, kmax, nrow) == adopted
    d = capi.DMatrix(device_ptr=ddata.data_ptr(), nrow=nrow, ncol=ncol, missing=-999.0)
    assert d.grid() == (0, 0, 0, False)                        # nobody has looked yet
    assert d.infer_grid() == (adopted != 0)
    assert d.grid() == ((adopted, 1, 0, True) if adopted else (0, 0, 0, False)), case
    d.free()
    # a subset of the columns, one at a time: the same words
    for c, col in enumerate(cols[:2]):
        one = _dev(torch, np.concatenate([np.zeros(kmax - 1, dtype=np.uint32), np.full(GUARD, PATTERN, dtype=np.uint32)]))
        synth.probe_detect_period(ddata, nrow, ncol, [col], kmax, one)
        torch.cuda.synchronize()
        one = _host_u32(one)
        assert np.array_equal(one[:kmax - 1], want[c]) and (one[kmax - 1:] == PATTERN).all(), (case, col)


# ---- the wiring in the product ----

VERDICT = re.compile(r"cluster verdict: (\S+) % of the rows take the first three decisions of the row before them, "
                     r"(\S+) % would by chance: order (\S+) -> (\w+)")


def test_the_product_judges_the_rows_as_the_reference_does(tmp_path):
    """One fresh process with OHX_DEBUG=1 predicts 2^18 + 1000 device-resident rows three times with ohx_cluster on
    auto (tests/cluster_support.py wiring_child): rows in grid order from a ragged shard are left, the same rows
    shuffled are clustered, and so are rows under a booster whose first tree is a root leaf (order 0.00).  The
    percentages it prints are the reference's, and the margins the oracle's."""
    out = tmp_path / "margins.npz"
    env = dict(os.environ, OHX_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", "import sys; from tests import cluster_support as K; K.wiring_child(sys.argv[1])",
                        str(out)], cwd=helpers.ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    said = VERDICT.findall(r.stderr)
    assert len(said) == 3, r.stderr[-4000:]
    got = np.load(out)
    for i, ((name, rows), line, expect) in enumerate(zip(K.wiring_batches(), said, ("leave", "cluster", "cluster")), 1):
        image, trees, heads = K.booster(name)
        lead = K.keys(trees, heads, rows, S.NFEAT, synth.XX_MISS, 1, 1, 0)           # one tree, one step: the lead
        order, observed, by_chance = K.order(K.agree(lead, len(rows)), len(rows))
        assert line == ("%.1f" % (100.0 * observed), "%.1f" % (100.0 * by_chance), "%.2f" % order, expect), (name, line)
        assert (order < 0.33) == (expect == "cluster")
        want = helpers.oracle_predict(synth.convert_model(image, "binary"), rows, synth.XX_MISS)
        assert np.array_equal(helpers.bits(got["margins_%d" % i]), helpers.bits(want)), name
    assert said[2][2] == "0.00" and said[2][1] == "100.0"
