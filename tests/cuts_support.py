"""Shared by the device-cuts tests: the column kinds a radix select can go wrong on, and the comparison with the numpy
restatement of the header (tests/grow_support.quantile_cuts).  Nothing here calls the code under test."""
import numpy as np

from tests import grow_support as G
from tests import helpers

KINDS = ("normal", "low mantissa bits", "both signs", "zeros of both signs", "denormals", "constant", "all missing",
         "nan, -999 and inf mixed", "max_bins distinct", "max_bins + 1 distinct", "60 % zeros")


def columns(n, max_bins, missing, seed=0):
    """-> float32 [n][len(KINDS)], one column per kind of KINDS."""
    rng = np.random.default_rng(seed + 1000 * n + max_bins)
    x = np.zeros((n, len(KINDS)), dtype=np.float32)
    x[:, 0] = rng.normal(3, 10, n)
    # 1.0 + k * 2^-23, k < 1024: the first 22 key bits agree, all three passes decide
    x[:, 1] = (np.uint32(0x3F800000) + rng.integers(0, 1024, n).astype(np.uint32)).view(np.float32)
    x[:, 2] = rng.normal(0, 1, n) * np.exp(rng.normal(0, 8, n))
    x[:, 3] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30], np.float32), n)
    x[:, 4] = (rng.integers(0, 600, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    x[:, 5] = -2.5
    x[:, 6] = missing
    v = rng.normal(0, 1, n).astype(np.float32)
    pick = rng.integers(0, 8, n)
    v[pick == 0] = np.nan
    v[pick == 1] = -999.0
    v[pick == 2] = np.inf
    v[pick == 3] = -np.inf
    x[:, 7] = v
    x[:, 8] = rng.integers(0, max_bins, n) * 0.5 - 3
    x[:min(n, max_bins), 8] = np.arange(min(n, max_bins)) * 0.5 - 3
    x[:, 9] = rng.integers(0, max_bins + 1, n) * 0.25 - 7
    x[:min(n, max_bins + 1), 9] = np.arange(min(n, max_bins + 1)) * 0.25 - 7
    x[:, 10] = np.where(rng.random(n) < 0.6, 0.0, rng.normal(0, 1, n))
    return x


def same_cuts(got, x, missing, max_bins, what=""):
    """Asserts that got = (cut_ptr, cut_values) is what the header says for the sample x: pointers equal, values equal
    (array_equal: a zero of either sign equals a zero), and no returned cut is a negative zero."""
    ptr, vals = got
    wptr, wvals = G.quantile_cuts(x, missing, max_bins)
    assert np.array_equal(ptr, wptr), (what, ptr, wptr)
    assert np.array_equal(vals, wvals), (what, np.flatnonzero(vals != wvals)[:8])
    assert not np.any(helpers.bits(vals) == np.uint32(0x80000000)), (what, "a cut is -0.0")
