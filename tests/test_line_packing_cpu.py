"""The placement of the super-node groups by cache line ("ohx_super_pack" 0..3, csrc/flatten.hpp kSuperPack*) on the
host: for every variant and every shape of tests/line_packing_support.py the layout walked the kernels' way gives the
oracle's margins bit for bit, emit_super's arrays keep what flatten.hpp promises, the trees start on a line and sibling
records' child groups share one; and the host line counter (csrc/line_count.cpp) counts what it says on forests small
enough to count by hand."""
import functools

import numpy as np
import pytest

from quickchem_amd import synth
from tests import booster_shapes as S
from tests import helpers
from tests import line_packing_support as L

NAMES = ("stump", "left", "right", "complete", "parity", "phases", "cap")
MISSING = -999.0


@functools.lru_cache(maxsize=None)
def world():
    """rows (NaN, -999.0, +-0, denormals, +-3e38 among them: test_random_forests.random_rows), the boosters whose
    thresholds are those rows' values, and per booster the rows with tie rows led down its trees, and the oracle's
    margins - computed once"""
    rng = np.random.default_rng(11)
    from tests.test_random_forests import random_rows
    base = random_rows(rng, 2000, S.NFEAT)
    forests = L.make_forests(base, which=NAMES)
    out = {}
    for name, (js, trees) in forests.items():
        finite = np.where(np.isfinite(base) & (base != np.float32(MISSING)), base, np.float32(0.5))
        rows = np.ascontiguousarray(np.concatenate([base, S.tie_rows(rng, trees, 1500, base=finite)]), dtype=np.float32)
        out[name] = (js, trees, rows, helpers.oracle_predict(synth.convert_model(js, "binary"), rows, MISSING))
    return out


def test_the_rows_hold_what_they_should():
    rows = world()["complete"][2]
    assert np.isnan(rows).any() and (rows == np.float32(MISSING)).any() and (np.abs(rows) >= np.float32(3e38)).any()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("pack", L.PACKS)
def test_walk_matches_the_oracle_and_the_layout_keeps_its_promises(name, pack):
    js, trees, rows, want = world()[name]
    got, info = synth.super_walk_cpu(js, rows, MISSING, super_pack=pack)
    assert got is not None, "the booster lost its super-nodes"
    assert np.array_equal(helpers.bits(got), helpers.bits(want))
    rec = synth.super_records_cpu(js, pack)
    assert info["super_nodes"] == len(rec["nodes"])
    by_line, pairs = L.check_layout(rec, pack, may_fall_back=(name == "cap"))
    if name == "cap":
        # 15 724 groups breadth first; the pairs leave out at most one number, the families' stretches a third of the last
        # level's 4 800: past the 14 bits of a group index, so that variant numbers the tree the old way
        old = (len(synth.super_records_cpu(js, 0)["nodes"]) - 48) // 4
        assert old == 15724 and old <= L.MAX_GROUPS
        assert by_line == (1 if pack == 2 else 0)
        assert (len(rec["nodes"]) - 48) // 4 <= old + 1
    elif pack >= 2:
        assert by_line == len(trees)
    if pack >= 2 and name in ("complete", "phases", "parity") or (pack == 2 and name == "cap"):
        assert pairs > 0
    # records: the bases cost at most a group a tree, the pairs at most one more
    old = len(synth.super_records_cpu(js, 0)["nodes"])
    if pack in (1, 2):
        assert len(rec["nodes"]) <= old + 8 * len(trees)


def test_base_parity_pads_one_group():
    """odd, odd, even group counts: breadth first the second tree starts on an odd group and the third on an even one;
    with bases on lines the second tree moved by one group and the third by two."""
    js = world()["parity"][0]
    old, new = synth.super_records_cpu(js, 0)["heads"][:, 0], synth.super_records_cpu(js, 1)["heads"][:, 0]
    assert [int(b) // 4 % 2 for b in old] == [0, 1, 0]
    assert [int(b) for b in new - old] == [0, 4, 8]


def test_chains_pair_their_singles():
    """a chain's deep groups are all singles (one child goes on): each takes the half line the one before left open, so
    the numbers stay dense and consecutive levels share a line"""
    for name in ("left", "right"):
        js = world()[name][0]
        a, b = synth.super_records_cpu(js, 0), synth.super_records_cpu(js, 2)
        assert len(b["nodes"]) - len(a["nodes"]) in (0, 4)


# ---- the line counter ----

def hand_forest():
    """A complete depth-5 tree (leaves at an odd depth: phase 0) that splits on feature 0 at 0.0 at the root and on
    feature 1 at 0.0 everywhere else: the root's record at slot 4, the four records of step 2 in group 2 (slots 8 - 11:
    one line), those of step 3 in groups 3 - 6 (slots 12 - 27: group 3 in the line of group 2, 4 and 5 in the next)."""
    t = L._complete_tree(5)
    for n in range(len(t.left)):
        if t.left[n] != -1:
            t.feat[n], t.cond[n], t.dl[n] = (0 if n == 0 else 1), 0.0, 0
        else:
            t.cond[n] = 0.25
    S._force_phase(np.random.default_rng(0), t, 0)
    return S.booster_json([t], 0.0)


@pytest.mark.parametrize("pack", L.PACKS)
def test_line_counter_on_a_forest_counted_by_hand(pack):
    js = hand_forest()
    assert synth.super_heads_cpu(js).tolist() == [[0, 3]]
    same = np.full((1, 64, S.NFEAT), -1.0, dtype=np.float32)
    table, info = synth.super_line_count(js, same, pack, first_step=0)
    assert sorted(table) == [0, 1, 2]
    for s in range(3):                      # 64 identical rows: one record, one line, one look-up per quad
        assert (table[s]["gathers"], table[s]["records"], table[s]["lines"], table[s]["lookups"]) == (1, 1.0, 1.0, 16.0)
    assert info["records"] == 4 * 7 + 48 and info["fillers"] == 4 + 3 + 48
    # the rows part at the root, half and half: records 4 | 8, 10 (one group) | 12, 20 (groups 3 and 5: two lines)
    split = same.copy()
    split[0, 32:, 0] = 1.0
    table, _ = synth.super_line_count(js, split, pack, first_step=0)
    assert [table[s]["records"] for s in range(3)] == [1.0, 2.0, 2.0]
    assert [table[s]["lines"] for s in range(3)] == [1.0, 1.0, 2.0]
    assert [table[s]["lookups"] for s in range(3)] == [16.0, 16.0, 16.0]
    # ... lane by lane instead: every quad holds both, and a brick's lane order moves nothing between the halves
    split = same.copy()
    split[0, 1::2, 0] = 1.0
    table, _ = synth.super_line_count(js, split, pack, first_step=0)
    assert [table[s]["lookups"] for s in range(3)] == [16.0, 16.0, 32.0]
    assert [table[s]["lines"] for s in range(3)] == [1.0, 1.0, 2.0]
    # a brick of 4 x 4 x 4, k fastest: lane l holds gridcell (i, j, k) = (l / 4 % 4, l / 16, l % 4), so rows that part by
    # k (grid order: cell = i + 4 j + 16 k) part inside every quad, and rows that part by j do in no quad
    by_k = same.copy()
    by_k[0, 32:, 0] = 1.0                   # k >= 2
    table, _ = synth.super_line_count(js, by_k, pack, brick=(2, 2, 2), k_fastest=True, first_step=0)
    assert table[2]["lookups"] == 32.0
    table, _ = synth.super_line_count(js, by_k, pack, brick=(2, 2, 2), k_fastest=False, first_step=0)
    assert table[2]["lookups"] == 16.0
    # 16 tiles of a block, half of them on either side: two lines for the block, one for every wave
    block = np.repeat(same, 16, axis=0)
    block[8:, :, 0] = 1.0
    table, _ = synth.super_line_count(js, block, pack, first_step=0)
    assert (table[2]["gathers"], table[2]["lines"], table[2]["block_lines"]) == (16, 1.0, 2.0)
