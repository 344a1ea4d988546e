"""Timing of a booster with categorical splits (docs/14_categorical.md) against its numeric twin, in one process.

The booster is the benchmark's (100 trees of depth <= 18, 27 features) with the splits on CAT_FEATURES made categorical:
the column is binned into categories 0 .. M over its range, a split `x < thr` becomes the suffix set {k, ..., M} with k
the bin of thr, and the rows' column holds the bin of its value - so rows, tree shapes and the coherence of neighbouring
rows stay the benchmark's.  The numeric twin has `x < float(k)` at the same nodes and routes every row identically
(tests/categorical_support.py); it is the model the kernels of the commit before this feature can walk.  Two variants:
M = 31 (every set inline in its node) and M = 95 (every set three words beside the nodes).

Measured, per variant, on the C360 L72 rows resident in HBM through OHXBoosterPredictDevice (device events around each
call, medians of --reps calls after --warmup):
  1. the twin through ohx_kernel = wide: the direct kernel without LDS - what a minimal implementation amounts to;
  2. the twin through the default kernel;
  3. the categorical booster through the new tile kernel (and, for context, through the new direct kernel).
The margins of (1), (2) and (3) are compared bit for bit on the way.  Prints one JSON document; --out writes it too."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from quickchem_amd import capi, synth  # noqa: E402

CAT_FEATURES = (2, 9, 16, 23)


def time_calls(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "reps": reps}


def bin_of(x, lo, hi, M):
    return np.clip(np.floor((np.asarray(x, dtype=np.float64) - lo) / (hi - lo) * (M + 1)), 0, M)


def variants(image, ranges, M):
    """-> (categorical JSON, twin JSON, categorical nodes) from the benchmark booster's JSON image."""
    doc = json.loads(bytes(image))
    twin = json.loads(bytes(image))
    count = 0
    trees = doc["learner"]["gradient_booster"]["model"]["trees"]
    for t, tw in zip(trees, twin["learner"]["gradient_booster"]["model"]["trees"]):
        feat = np.array(t["split_indices"])
        inner = np.array(t["left_children"]) != -1
        cond = np.array(t["split_conditions"], dtype=np.float64)
        k_of = np.zeros(len(feat), dtype=np.int64)
        is_cat = np.zeros(len(feat), dtype=bool)
        for f in CAT_FEATURES:
            lo, hi = ranges[f]
            sel = inner & (feat == f)
            k_of[sel] = np.clip(bin_of(cond[sel], lo, hi, M), 1, M).astype(np.int64)
            is_cat |= sel
        nodes = [int(n) for n in np.flatnonzero(is_cat)]
        cats, segments, sizes = [], [], []
        for n in nodes:
            k = int(k_of[n])
            tw["split_conditions"][n] = float(k)
            t["split_conditions"][n] = float(k)              # a 1.6.0 writer puts NaN here; the reader takes either
            t["split_type"][n] = 1
            segments.append(len(cats))
            sizes.append(M + 1 - k)
            cats.extend(range(k, M + 1))
        t["categories_nodes"] = nodes
        t["categories_segments"], t["categories_sizes"], t["categories"] = segments, sizes, cats
        count += len(nodes)
    doc["learner"]["feature_types"] = ["c" if f in CAT_FEATURES else "float" for f in range(synth.NFEAT)]
    doc["learner"]["feature_names"] = list(synth.FEATURE_NAMES)
    return json.dumps(doc).encode(), json.dumps(twin).encode(), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grid", default="C360")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "categorical_timing needs the MI355X"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    base = synth.make_model(fmt="json")
    grid = synth.GRIDS[args.grid]
    n = grid[0] * grid[1] * grid[2]
    rows = torch.empty(n * synth.NFEAT, dtype=torch.float32, device="cuda")
    synth.rows_device(grid, 0, n, rows)
    torch.cuda.synchronize()
    view = rows.view(n, synth.NFEAT)
    ranges = {}
    for f in CAT_FEATURES:
        col = view[:, f]
        ok = col != synth.XX_MISS
        ranges[f] = (float(col[ok].min()), float(col[ok].max()))
    res = {"rows": n, "grid": args.grid, "cat_features": list(CAT_FEATURES), "ranges": ranges}
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    for label, M in (("inline_sets_M31", 31), ("three_word_sets_M95", 95)):
        cat_js, twin_js, count = variants(base.image, ranges, M)
        print("%s: models made, %d categorical nodes" % (label, count), file=sys.stderr, flush=True)
        binned = view.clone()
        for f in CAT_FEATURES:
            lo, hi = ranges[f]
            col = view[:, f]
            b = torch.clamp(torch.floor((col.double() - lo) / (hi - lo) * (M + 1)), 0, M).float()
            binned[:, f] = torch.where(col == synth.XX_MISS, col, b)
        d = capi.DMatrix(device_ptr=binned.data_ptr(), nrow=n, ncol=synth.NFEAT, missing=synth.XX_MISS)
        d.set_grid(grid[0], grid[1], 0)
        r = {"categorical_nodes": count}

        def run(image, params, key):
            b = capi.Booster(model_buffer=np.frombuffer(image, dtype=np.uint8).copy())
            for k, v in params:
                b.set_param(k, v)
            timing = time_calls(lambda: b.predict_device(d, out.data_ptr(), 1), args.warmup, args.reps)
            torch.cuda.synchronize()
            b.check()
            info = b.info()
            r[key] = {"kernel": b.kernel_symbols_for(d), "margin": timing, "node_slots": info["num_slots"],
                      "node_bytes": info["node_bytes"], "categorical_splits": b.num_categorical_splits()}
            got = out.clone()
            b.free()
            print("%s %s: %.2f ms (%s)" % (label, key, timing["median_ms"], r[key]["kernel"]), file=sys.stderr, flush=True)
            return got

        m1 = run(twin_js, [("ohx_kernel", "wide")], "1_twin_wide_direct")
        m2 = run(twin_js, [], "2_twin_default")
        m3 = run(cat_js, [], "3_categorical_tile")
        m4 = run(cat_js, [("ohx_cat_kernel", "direct")], "3b_categorical_direct")
        r["bit_identical"] = bool(torch.equal(m1.view(torch.int32), m2.view(torch.int32)) and
                                  torch.equal(m1.view(torch.int32), m3.view(torch.int32)) and
                                  torch.equal(m1.view(torch.int32), m4.view(torch.int32)))
        r["set_words"] = (r["3_categorical_tile"]["node_bytes"] - 16 * r["3_categorical_tile"]["node_slots"]) // 4
        r["tile_over_twin_wide"] = r["3_categorical_tile"]["margin"]["median_ms"] / r["1_twin_wide_direct"]["margin"]["median_ms"]
        r["tile_over_twin_default"] = r["3_categorical_tile"]["margin"]["median_ms"] / r["2_twin_default"]["margin"]["median_ms"]
        res[label] = r
        d.free()
        del binned
    res["seconds"] = time.perf_counter() - t0
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
