"""Timing of a multi-class booster (several output groups, docs/13_output_groups.md) against the single-output booster
of the benchmark, in the same process: a synthetic 3-class booster of 34 rounds x 3 = 102 trees of depth <= 18 (the
benchmark's generator, trees assigned to the classes round-robin, multi:softprob) and the 100-tree single-output
booster, both predicting the C360 L72 rows in HBM through OHXBoosterPredictDevice with the grid said.  Device events
around each call after a warm-up, median of --reps; prints one JSON document and writes it to --out if given.

Reports per booster: the margin call (option_mask 1) and, for the 3-class one, the probabilities (option_mask 0).  The
3-class walk covers about the same trees as the single-output one, in three launches over the same rows (one per
class), then group_finish reads three planes and writes [nrow][3]."""
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
    return {"median_ms": float(np.median(times)) * 1e3, "min_ms": float(np.min(times)) * 1e3, "reps": reps}


def three_class(image, K=3):
    doc = json.loads(bytes(image))
    learner = doc["learner"]
    n = len(learner["gradient_booster"]["model"]["trees"])
    learner["gradient_booster"]["model"]["tree_info"] = [t % K for t in range(n)]
    learner["learner_model_param"]["num_class"] = str(K)
    learner["learner_model_param"]["base_score"] = "0.5"
    learner["objective"] = {"name": "multi:softprob", "softmax_multiclass_param": {"num_class": str(K)}}
    return json.dumps(doc).encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "output_groups_timing needs the MI355X"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    single = synth.make_model()
    multi = three_class(synth.make_model(num_trees=102, fmt="json").image.tobytes())
    res = {"model_seconds": time.perf_counter() - t0}
    grid = synth.GRIDS["C360"]
    n = grid[0] * grid[1] * grid[2]
    rows = torch.empty(n * synth.NFEAT, dtype=torch.float32, device="cuda")
    synth.rows_device(grid, 0, n, rows)
    torch.cuda.synchronize()
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=n, ncol=synth.NFEAT, missing=synth.XX_MISS)
    d.set_grid(grid[0], grid[1], 0)
    res["rows"] = n
    out = torch.empty(n * 3, dtype=torch.float32, device="cuda")
    b1 = capi.Booster(model_buffer=single.image)
    b3 = capi.Booster(model_buffer=np.frombuffer(multi, dtype=np.uint8).copy())
    assert b1.num_groups == 1 and b3.num_groups == 3
    res["single_output_100_trees"] = {"kernel": b1.kernel_symbols_for(d),
                                      "margin": time_calls(lambda: b1.predict_device(d, out.data_ptr(), 1), args.warmup,
                                                           args.reps)}
    res["three_class_102_trees"] = {
        "kernel": b3.kernel_symbols_for(d),
        "margin": time_calls(lambda: b3.predict_device(d, out.data_ptr(), 1), args.warmup, args.reps),
        "softprob": time_calls(lambda: b3.predict_device(d, out.data_ptr(), 0), args.warmup, args.reps)}
    b1.check()
    b3.check()
    res["ratio_margin"] = res["three_class_102_trees"]["margin"]["median_ms"] / res["single_output_100_trees"]["margin"]["median_ms"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
