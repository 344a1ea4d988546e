"""Timing of the leaf refit (OHXBoosterRefitLeavesDevice) on the benchmark's synthetic OH booster (100 trees, depth <= 18,
as bench.py builds it) and the C360 L72 rows resident in HBM.  Labels = the margins of a booster of the same recipe
grown from another seed.  Run by hand on an MI355X; writes one JSON document (default profiles/refit_timing.json).

The whole call is timed from the host (it waits at its end), the median of `--reps` rounds after `--warmup`.  A round
loads a fresh booster and refits it twice: the first call also allocates the state's buffers (22 GB of leaf ids among
them), as a caller's first refit does; the second reuses them.  Both are recorded.  OHXBoosterCountVisitsDevice - the
same walk without the id stores - is timed on the same rows in the same process with device events, and the RMSE
against the labels is taken before and after through OHXBoosterPredictDevice.  (profiles/r14_refit_timing.json was
written while the library still held a second, lane-by-lane accumulate kernel behind a knob: its keys refit_lanes and
refit_merged are that comparison; the merged kernel is the one that was kept.)

The three kernels' own times come from a second run of this script under a kernel trace, with --reps 1 --warmup 0
(docs/17_leaf_refit.md 17.4 says how)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grid", default="C360", help="a name of synth.GRIDS")
    ap.add_argument("--label-seed", type=int, default=synth.MODEL_SEED + 1)
    ap.add_argument("--eta", type=float, default=1.0)
    ap.add_argument("--reg-lambda", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "refit_timing needs the MI355X"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    model = synth.make_model()
    teacher = synth.make_model(model_seed=args.label_seed)
    F = synth.NFEAT
    grid = synth.GRIDS[args.grid]
    n = grid[0] * grid[1] * grid[2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = synth.refit_plan(n, F, model.num_trees, cus)
    res = {"model": {"trees": model.num_trees, "nodes": model.num_nodes, "leaves": model.num_leaves,
                     "max_depth": model.max_depth}, "rows": n, "plan": plan, "eta": args.eta,
           "reg_lambda": args.reg_lambda, "reps": args.reps, "warmup": args.warmup,
           "model_seconds": time.perf_counter() - t0}
    rows = torch.empty((n, F), dtype=torch.float32, device="cuda")
    synth.rows_device(grid, 0, n, rows)
    stream = torch.cuda.current_stream().cuda_stream
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=n, ncol=F, missing=synth.XX_MISS)
    d.set_grid(grid[0], grid[1], 0)

    def margins(b):
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        b.predict_device(d, out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        b.check()
        return out

    tb = capi.Booster(model_buffer=teacher.image)
    labels = margins(tb)
    tb.free()

    def rmse(b):
        return float(torch.sqrt(torch.mean((margins(b).double() - labels.double()) ** 2)).item())

    b = capi.Booster(model_buffer=model.image)
    res["rmse_before"] = rmse(b)
    # the same walk without the id stores, on the same rows
    times = []
    for k in range(args.warmup + args.reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        b.count_visits_device(d, stream=stream)
        e.record()
        e.synchronize()
        if k >= args.warmup:
            times.append(a.elapsed_time(e) / 1e3)
    res["count_visits"] = {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times))}
    print("count_visits", json.dumps(res["count_visits"]), flush=True)
    b.free()

    times = []
    for k in range(args.warmup + args.reps):
        b = capi.Booster(model_buffer=model.image)
        # the state's buffers (22 GB of leaf ids among them) are allocated by the first call on a booster, as a
        # caller's first refit pays for them; the second call reuses them.  Both are recorded
        torch.cuda.synchronize()
        t = time.perf_counter()
        refit = b.refit_leaves_device(d, labels.data_ptr(), n, eta=args.eta, reg_lambda=args.reg_lambda, stream=stream)
        dt = time.perf_counter() - t
        t = time.perf_counter()
        b.refit_leaves_device(d, labels.data_ptr(), n, eta=args.eta, reg_lambda=args.reg_lambda, stream=stream)
        dt2 = time.perf_counter() - t
        if k >= args.warmup:
            times.append((dt, dt2))
        b.free()
    first, again = [x[0] for x in times], [x[1] for x in times]
    res["refit"] = {"first_call_median_s": float(np.median(first)), "median_s": float(np.median(again)),
                    "min_s": float(np.min(again)), "max_s": float(np.max(again)), "leaves_refit_first": refit,
                    "row_tree_adds_per_s": n * model.num_trees / float(np.median(again))}
    # the RMSE is taken of a booster refit once
    b = capi.Booster(model_buffer=model.image)
    b.refit_leaves_device(d, labels.data_ptr(), n, eta=args.eta, reg_lambda=args.reg_lambda, stream=stream)
    res["refit"]["rmse_after"] = rmse(b)
    b.free()
    print("refit", json.dumps(res["refit"]), flush=True)
    d.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
