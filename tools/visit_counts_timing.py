"""Timing of the node visit counts (OHXBoosterCountVisitsDevice) on the benchmark's synthetic OH booster (100 trees,
depth <= 18, grown on 2**20 cells, as bench.py builds it) and the C360 L72 rows resident in HBM with the grid said.
Run by hand on an MI355X.  Device events around each call, the median of `--reps` calls after `--warmup` calls; writes
one JSON document (default profiles/visit_counts_timing.json).

Three things are timed: "ohx_visits_kernel" = lds; "ohx_visits_kernel" = global (what auto takes); and the only
route to the same numbers the library had before - OHXBoosterPredictDevice with option_mask = 16 alone, on 2**20 rows where its [nrow][100] output
fits, a LOWER bound on that route (the leaf ids would still have to be counted).  The new call is timed on the same
2**20 rows as well.  The counts of the two routes are compared with each other, and on the 2**20 rows with a bincount
of the leaf ids, before anything is reported."""
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
        times.append(a.elapsed_time(b) / 1e3)
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times)),
            "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visit_counts_timing.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", default="C360", help="a name of synth.GRIDS")
    ap.add_argument("--small-rows", type=int, default=1 << 20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "visit_counts_timing needs the MI355X"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    model = synth.make_model()
    plan = synth.visits_plan(model.image)
    res = {"model": {"trees": model.num_trees, "nodes": model.num_nodes, "leaves": model.num_leaves,
                     "max_depth": model.max_depth},
           "plan": {"lds_trees": plan["lds_trees"], "hist_leaves": plan["hist_leaves"],
                    "lds_bytes_lds_kernel": plan["lds_bytes_lds"], "lds_bytes_global_kernel": plan["lds_bytes_global"]},
           "model_seconds": time.perf_counter() - t0, "reps": args.reps, "warmup": args.warmup}
    F = synth.NFEAT
    grid = synth.GRIDS[args.grid]
    n = grid[0] * grid[1] * grid[2]
    rows = torch.empty((n, F), dtype=torch.float32, device="cuda")
    synth.rows_device(grid, 0, n, rows)
    stream = torch.cuda.current_stream().cuda_stream

    def counts_of(kernel, dmat, nrow):
        b = capi.Booster(model_buffer=model.image)
        b.set_param("ohx_visits_kernel", kernel)
        r = time_calls(lambda: b.count_visits_device(dmat, stream=stream), args.warmup, args.reps)
        counts, seen = b.visit_counts(stream=stream)
        assert seen == nrow * (args.warmup + args.reps)
        b.free()
        r.update({"rows": nrow, "rows_per_s": nrow / r["median_s"],
                  "increments_per_s": nrow * model.num_trees / r["median_s"]})
        return r, counts

    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=n, ncol=F, missing=synth.XX_MISS)
    d.set_grid(grid[0], grid[1], 0)
    res["lds_" + args.grid], c_auto = counts_of("lds", d, n)
    print("lds", json.dumps(res["lds_" + args.grid]), flush=True)
    res["global_" + args.grid], c_global = counts_of("global", d, n)
    print("global", json.dumps(res["global_" + args.grid]), flush=True)
    assert all(np.array_equal(a, g) for a, g in zip(c_auto, c_global)), "the two routes disagree"
    assert all(int(c[0]) == n * (args.warmup + args.reps) for c in c_auto)
    d.free()

    # the same 2**20 rows three ways
    m = min(args.small_rows, n)
    ds = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=m, ncol=F, missing=synth.XX_MISS)
    ds.set_grid(grid[0], grid[1], 0)
    b = capi.Booster(model_buffer=model.image)
    ids = torch.empty((m, model.num_trees), dtype=torch.float32, device="cuda")
    res["leaf_ids_small"] = time_calls(lambda: b.predict_device(ds, ids.data_ptr(), option_mask=16, stream=stream),
                                       args.warmup, args.reps)
    res["leaf_ids_small"].update({"rows": m, "output_bytes": m * model.num_trees * 4})
    print("leaf ids", json.dumps(res["leaf_ids_small"]), flush=True)
    res["lds_small"], c_small = counts_of("lds", ds, m)
    res["global_small"], _ = counts_of("global", ds, m)
    res["lds_small"]["vs_leaf_ids"] = res["lds_small"]["median_s"] / res["leaf_ids_small"]["median_s"]
    res["global_small"]["vs_leaf_ids"] = res["global_small"]["median_s"] / res["leaf_ids_small"]["median_s"]
    print("lds small", json.dumps(res["lds_small"]), "global small", json.dumps(res["global_small"]), flush=True)
    # the counted leaves are the leaf ids' (one tree is enough on the host: the tests hold every tree to this)
    host_ids = ids[:, 0].to(torch.int64)
    per_call = torch.bincount(host_ids, minlength=len(c_small[0])).cpu().numpy().astype(np.uint64)
    leaves = per_call != 0
    assert np.array_equal(c_small[0][leaves], per_call[leaves] * np.uint64(args.warmup + args.reps)), "tree 0's counts"
    ds.free()
    b.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
