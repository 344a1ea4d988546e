"""The clustering key's two restatements against each other, and the two host decisions of the clustering pass and the
level search (csrc/kernels.hpp cluster_order, pick_level_period) against what tests/cluster_support.py writes down.
No GPU: what the kernels make of the same cases is tests/test_gpu_cluster.py."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from quickchem_amd import synth
from tests import booster_shapes as S
from tests import cluster_support as K
from tests import helpers
from tests.test_adversarial_boosters_cpu import MISSING

BOOSTERS = (1, 2, 3, 5, 135, "synth")


def _shapes(ntree):
    return [s for s in K.KEY_SHAPES if s[0] <= ntree]


def test_the_cases_reach_the_key_walks_edges():
    """From emit_super's own heads and the reference walk, before anything is compared: a root leaf among the key's
    trees, both phases as tree 0, a key tree that runs out of steps before the key does, rows that stand on a leaf
    from some step on, and rows that reach their leaf after the first decision of a record."""
    root_leaf = short = False
    phases0 = set()
    stats = {}
    for name in BOOSTERS:
        image, trees, heads = K.booster(name)
        phases0.add(int(heads[0][0]))
        for ntrees, nsteps, _ in _shapes(len(trees)):
            root_leaf |= any(K.is_root_leaf(t) for t in trees[:ntrees])
            short |= bool((heads[:ntrees, 1] < nsteps).any())
        rows = K.rows(name, -999.0)
        K.keys(trees, heads, rows, S.NFEAT, -999.0, min(2, len(trees)), 7, 0, stats=stats)
    assert root_leaf and short and phases0 == {0, 1}, (root_leaf, short, phases0)
    assert stats["leaf_after_b0"] > 0 and stats["on_a_leaf"] > 0, stats


def test_the_tie_rows_sit_on_thresholds_the_key_decides_at(monkeypatch):
    """A key walk that read < as <= would move some of the tie rows (the second half of the rows), for every booster
    with a split and every key shape the GPU tests use."""
    for name in BOOSTERS[1:]:
        _, trees, heads = K.booster(name)
        rows = K.rows(name, -999.0)
        for ntrees, nsteps, zorder in _shapes(len(trees)):
            if all(K.is_root_leaf(t) for t in trees[:ntrees]):
                continue
            monkeypatch.setattr(K, "_LESS", np.less)
            want = K.keys(trees, heads, rows, S.NFEAT, -999.0, ntrees, nsteps, zorder)
            monkeypatch.setattr(K, "_LESS", np.less_equal)
            loose = K.keys(trees, heads, rows, S.NFEAT, -999.0, ntrees, nsteps, zorder)
            assert (loose[1500:] != want[1500:]).any(), (name, ntrees, nsteps, zorder)


@pytest.mark.parametrize("name", BOOSTERS)
def test_the_two_key_restatements_agree(name):
    """The key from the trees and the key from emit_super's records, for every placement of the records, every missing
    marker and every key shape.  The key does not depend on the placement."""
    image, trees, heads = K.booster(name)
    records = [synth.super_records_cpu(image, pack) for pack in synth.SUPER_PACKS]
    assert all(r is not None for r in records)
    differ_by_pack = False
    for missing in MISSING:
        rows = K.rows(name, missing)
        assert len(rows) == 3000 and np.isfinite(rows[1500:]).all()
        if np.isinf(missing):
            assert np.isposinf(rows).any() and np.isneginf(rows).any() and np.isnan(rows).any()
        for ntrees, nsteps, zorder in _shapes(len(trees)):
            want = K.keys(trees, heads, rows, S.NFEAT, missing, ntrees, nsteps, zorder)
            for pack, rec in zip(synth.SUPER_PACKS, records):
                assert np.array_equal(rec["heads"][:, 3], heads[:, 1]) and \
                    np.array_equal((rec["heads"][:, 1] >> 8) & 1, heads[:, 0])
                got = K.keys_from_records(rec["nodes"], rec["heads"], rows, S.NFEAT, missing, ntrees, nsteps, zorder)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (name, missing, ntrees, nsteps, zorder, pack, bad[:5], got[bad[:5]], want[bad[:5]])
            differ_by_pack |= any(not np.array_equal(records[0]["nodes"], r["nodes"]) for r in records[1:])
    assert differ_by_pack or len(trees) < 5, "the placements are different arrays (else this checks nothing)"


@pytest.mark.parametrize("ncol", (26, 20, 16, 3, 2, 1))
def test_the_restatements_agree_on_narrow_matrices(ncol):
    """Columns at or beyond ncol are missing: every decision on them goes by the node's default."""
    image, trees, heads = K.booster(135)
    rec = synth.super_records_cpu(image, 2)
    for missing in (-999.0, float("nan")):
        rows = np.ascontiguousarray(K.rows(135, missing)[:, :ncol])
        for ntrees, nsteps, zorder in ((2, 7, 0), (4, 3, 1)):
            want = K.keys(trees, heads, rows, ncol, missing, ntrees, nsteps, zorder)
            got = K.keys_from_records(rec["nodes"], rec["heads"], rows, ncol, missing, ntrees, nsteps, zorder)
            assert np.array_equal(got, want)
            full = K.keys(trees, heads, K.rows(135, missing), S.NFEAT, missing, ntrees, nsteps, zorder)
            assert not np.array_equal(full, want), "the dropped columns decide something"


def test_a_filler_read_like_a_record_moves_rows_that_hold_plus_inf_in_feature_0():
    """What the key kernel did until this file existed: past its leaf a walk stands on fillers (feature 0 against +inf,
    csrc/flatten.cpp), and a row whose feature 0 IS +inf - a value, where the marker is -inf - went right there: 11
    where the key says 00.  Read that way the records give another key for exactly those rows; the kernel now stays on
    its leaf (tests/test_gpu_cluster.py holds it to that)."""
    image, trees, heads = K.booster(3)              # a stump and a chain: leaves long before the trip count
    rec = synth.super_records_cpu(image, 2)
    for missing, moves in ((float("-inf"), True), (float("inf"), False), (-999.0, False)):
        rows = K.rows(3, missing)
        want = K.keys(trees, heads, rows, S.NFEAT, missing, 2, 7, 0)
        walked = K.keys_from_records(rec["nodes"], rec["heads"], rows, S.NFEAT, missing, 2, 7, 0, fillers="walk")
        bad = walked != want
        assert bad.any() == moves
        assert not (bad & ~np.isposinf(rows[:, 0])).any()


def test_leads_and_agree_on_hand_made_keys():
    # plain (2, 7): tree 0's part is the top 15 bits of 30; z-order: root bits 29, 28, step 0 of tree 0 bits 27, 26
    key = np.array([0b101 << 27, 0b011 << 27 | 0x3FFFFFF, 0], dtype=np.uint32)
    assert K.leads(key, 2, 7, 0).tolist() == [5, 3, 0]
    z = np.array([1 << 29 | 0b10 << 26, 1 << 28 | 0b11 << 24, 0b01 << 26], dtype=np.uint32)
    assert K.leads(z, 2, 7, 1).tolist() == [6, 0, 1]
    assert K.leads(np.array([0b110], dtype=np.uint32), 1, 1, 0).tolist() == [6]
    # 130 rows of one outcome: all agree but rows 0, 64 and 128
    assert K.agree(np.full(130, 3, dtype=np.uint32), 130).tolist() == [127, 0, 0, 0, 130, 0, 0, 0, 0]
    alt = np.arange(200, dtype=np.uint32) % 2
    assert K.agree(alt, 200).tolist() == [0, 100, 100, 0, 0, 0, 0, 0, 0]


# ---- the rows' order ----

def _same(words, nrow):
    order, observed, by_chance, on = synth.cluster_order(words, nrow)
    want = K.order(words, nrow)
    assert (order, observed, by_chance) == want, (words, nrow)         # the same operations in the same order
    return order, on


def test_cluster_order_on_hand_made_words():
    n = 1 << 18
    # every row takes one outcome: nothing to tell order from - by chance 1, order 0, and the rows are clustered
    order, on = _same([n - n // 64, 0, 0, n, 0, 0, 0, 0, 0], n)
    assert order == 0.0 and on
    # a perfect 8-way split in eight runs: every row but a wave's first agrees with the one before
    order, on = _same([n - n // 64] + [n // 8] * 8, n)
    assert abs(order - (63 / 64 - 1 / 8) / (7 / 8)) < 1e-12 and order > 0.98 and not on
    # rows in no order: neighbours agree as often as chance has it
    order, on = _same([int(n * 63 / 64 / 8)] + [n // 8] * 8, n)
    assert abs(order) < 0.01 and on
    # ... and with unequal shares
    shares = [n // 2, n // 4, n // 8, n // 16, n // 32, n // 64, n // 128, n // 128]
    chance = sum((s / n) ** 2 for s in shares)
    order, on = _same([int(n * chance)] + shares, n)
    assert abs(order) < 0.01 and on
    # fewer agree than chance: below zero, clustered
    order, on = _same([0] + [n // 8] * 8, n)
    assert order < -0.14 and on
    # nearly one outcome, by chance just below 0.999: still judged - and below zero, since a wave's first row sits
    # out and the rows that can agree are 63 of 64
    few = 200
    order, on = _same([n - n // 64 - 2 * few, n - few, few, 0, 0, 0, 0, 0, 0], n)
    assert 0.998 < K.order([0, n - few, few, 0, 0, 0, 0, 0, 0], n)[2] < 0.999 and order < -1.0 and on


@pytest.mark.parametrize("n,shares", [(80008, None), (1 << 18, None), (300001, (100000, 100001, 50000, 25000, 12500, 6250, 3125, 3125))])
def test_the_order_rule_flips_between_two_neighbouring_counts(n, shares):
    """order < kClusterOrderBelow clusters: the count of agreeing rows at which the exact rational order passes 33/100,
    and the count one row below it."""
    shares = [n // 8] * 8 if shares is None else list(shares)
    assert sum(shares) == n
    chance = sum(Fraction(s, n) ** 2 for s in shares)
    exact = lambda h0: (Fraction(h0, n) - chance) / (1 - chance)      # noqa: E731
    h0 = next(h for h in range(n) if exact(h) >= Fraction(33, 100))
    assert exact(h0) != Fraction(33, 100) and exact(h0 - 1) < Fraction(33, 100)     # (no tie with the constant)
    below, on_below = _same([h0 - 1] + shares, n)
    above, on_above = _same([h0] + shares, n)
    assert below < 0.33 <= above
    assert on_below and not on_above


# ---- the adopted level size ----

def _verdict(kmax, fill=1):
    return np.full((4, kmax - 1), fill, dtype=np.uint32)


def test_pick_level_period_column_order_comes_before_the_smallest_period():
    nrow, kmax = 12 * 4096, 12
    v = _verdict(kmax)
    v[0, kmax - 2] = 0          # column 0: two levels of 24576
    v[1, kmax - 12] = 0         # column 1: twelve levels of 4096 - smaller, but a later column
    assert synth.pick_level_period(v, kmax, nrow) == 24576
    v[0, kmax - 2] = 1
    assert synth.pick_level_period(v, kmax, nrow) == 4096
    # within a column the smallest period that holds
    v = _verdict(kmax)
    for k in (2, 3, 4, 6, 12):
        v[2, kmax - k] = 0
    assert synth.pick_level_period(v, kmax, nrow) == 4096
    v[2, kmax - 12] = 1
    assert synth.pick_level_period(v, kmax, nrow) == 8192
    # the last word of the last column is read, and nothing behind it
    v = _verdict(kmax)
    v[3, kmax - 2] = 0
    assert synth.pick_level_period(v, kmax, nrow) == 24576
    # kmax 2: one word a column
    assert synth.pick_level_period([[1], [2], [0], [1]], 2, 8192) == 4096


def test_pick_level_period_never_adopts_words_1_and_2():
    kmax, nrow = 9, 9 * 4096
    for fill in (1, 2, 3, 0xFFFFFFFF):
        assert synth.pick_level_period(_verdict(kmax, fill), kmax, nrow) == 0
    v = _verdict(kmax, 2)
    v[:, ::2] = 1
    assert synth.pick_level_period(v, kmax, nrow) == 0
    v[1, kmax - 3] = 0
    assert synth.pick_level_period(v, kmax, nrow) == 3 * 4096


def test_pick_level_period_skips_a_period_that_does_not_fit_an_int():
    nrow, kmax = 1 << 33, 8
    v = _verdict(kmax, 0)                       # everything "periodic"
    # k = 8 and 4 give 2^30 and 2^31: the first fits, ascending periods
    assert synth.pick_level_period(v, kmax, nrow) == 1 << 30
    v[:, :] = 1
    v[0, kmax - 4] = 0                         # 2^31 = 0x80000000: one too many
    v[0, kmax - 2] = 0
    assert synth.pick_level_period(v, kmax, nrow) == 0
    v[1, kmax - 7] = 0                          # floor(2^33 / 7) fits
    assert synth.pick_level_period(v, kmax, nrow) == (1 << 33) // 7
    v = _verdict(2, 0)
    assert synth.pick_level_period(v, 2, 2 * 0x7FFFFFFF) == 0x7FFFFFFF
    assert synth.pick_level_period(v, 2, 2 * 0x80000000) == 0


# ---- the host functions under sanitizers ----

def test_the_host_decisions_under_sanitizers(tmp_path):
    """tools/cluster_host_check.cpp, a program of its own built with AddressSanitizer + UBSan (CPU only)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(helpers.ROOT, "quickchem_amd", "csrc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"       # kernels.hpp reads the HIP runtime's API header
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    if not os.path.exists(os.path.join(include, "hip", "hip_runtime_api.h")):
        include = "/opt/rocm/include"
    exe = tmp_path / "cluster_host_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", src, "-I", include,
                            os.path.join(helpers.ROOT, "tools", "cluster_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert re.search(r"\d+ orders, \d+ picks, 0 failures", r.stdout), r.stdout
