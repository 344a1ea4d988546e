"""Timing of per-feature contributions (OHXBoosterPredictContribsDevice) on the benchmark's synthetic OH booster
(100 trees, depth <= 18, grown on 2**20 cells, as bench.py builds it).  Device events around each call after a
warm-up; writes one JSON document (default profiles/contribs_timing.json).

Reports: exact contributions per second on a 48 x 24 x 72 rank block and on 4 096 rows; approximate mode on the
whole C360 L72 batch beside the margin predict of the same rows in the same process; the path table's bytes and
sum over paths of (len + 1)^2, and the least time the exact kernel's recurrences could take on the chip at the
VALU-instruction counts per element step read off the kernel's ISA (contribs.hip, gfx950, `hipcc --save-temps`):
every guarded step of the unrolled unwound sum is 8 VALU instructions; a step of the extend recurrence is 5 by the
source's arithmetic (three multiplies and an add for the weight that moves up, two multiplies for the one that stays,
with -ffp-contract=off) - a path of d distinct features takes d(d+1)/2 extend steps and d^2 unwound steps."""
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

# MI355X: 256 CUs x 4 SIMDs, a wave64 VALU instruction issues in 2 cycles at up to 2.4 GHz
VALU_WAVE_ISSUES_PER_S = 256 * 4 * 2.4e9 / 2


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
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contribs_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--extend-valu", type=float, default=5.0, help="VALU instructions per extend step")
    ap.add_argument("--unwind-valu", type=float, default=8.0, help="VALU instructions per unwound-sum step")
    ap.add_argument("--skip-c360", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "contribs_timing needs the MI355X"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    model = synth.make_model()
    st = synth.contribs_table_stats(model.image)
    res = {"model": {"trees": model.num_trees, "nodes": model.num_nodes, "leaves": model.num_leaves,
                     "max_depth": model.max_depth},
           "path_table": st, "model_seconds": time.perf_counter() - t0}
    b = capi.Booster(model_buffer=model.image)
    F = synth.NFEAT

    def exact_case(name, grid, nrow):
        rows = torch.empty((nrow, F), dtype=torch.float32, device="cuda")
        synth.rows_device(grid, 0, nrow, rows)
        out = torch.empty((nrow, F + 1), dtype=torch.float32, device="cuda")
        d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=nrow, ncol=F, missing=synth.XX_MISS)
        t = time.perf_counter()
        b.predict_contribs_device(d, out.data_ptr())          # builds the tables (timed apart)
        torch.cuda.synchronize()
        first = time.perf_counter() - t
        r = time_calls(lambda: b.predict_contribs_device(d, out.data_ptr()), 0, args.reps)
        r.update({"rows": nrow, "rows_per_s": nrow / r["median_s"], "first_call_s": first,
                  "chip_us_per_row": r["median_s"] / nrow * 1e6})
        # local accuracy on what was timed
        margin = torch.empty(nrow, dtype=torch.float32, device="cuda")
        b.predict_device(d, margin.data_ptr(), option_mask=1)
        torch.cuda.synchronize()
        o = out.double()
        err = (o.sum(dim=1) - margin.double()).abs() / (1.0 + o.abs().sum(dim=1))
        r["local_accuracy_max_rel"] = float(err.max())
        # sum over paths of d^2 and d, from sum (d + 1)^2, the element count (sum d) and the path count
        sum_d = st["elements"]
        sum_d2 = st["sum_len1_sq"] - 2 * sum_d - st["paths"]
        per_wave = args.extend_valu * (sum_d2 + sum_d) / 2 + args.unwind_valu * sum_d2
        bound = -(-nrow // 64) * per_wave / VALU_WAVE_ISSUES_PER_S
        r.update({"valu_per_wave": per_wave, "valu_bound_s": bound, "share_of_valu_bound": bound / r["median_s"]})
        d.free()
        res[name] = r
        print(name, json.dumps(r), flush=True)

    exact_case("exact_rank_block_48x24x72", (48, 24, 72), 48 * 24 * 72)
    exact_case("exact_4096_rows", synth.GRIDS["C12"], 4096)
    if not args.skip_c360:
        grid = synth.GRIDS["C360"]
        n = grid[0] * grid[1] * grid[2]
        rows = torch.empty((n, F), dtype=torch.float32, device="cuda")
        synth.rows_device(grid, 0, n, rows)
        d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=n, ncol=F, missing=synth.XX_MISS)
        d.set_grid(grid[0], grid[1], 0)
        margin = torch.empty(n, dtype=torch.float32, device="cuda")
        pred = time_calls(lambda: b.predict_device(d, margin.data_ptr()), 2, max(args.reps, 5))
        out = torch.empty((n, F + 1), dtype=torch.float32, device="cuda")
        approx = time_calls(lambda: b.predict_contribs_device(d, out.data_ptr(), approximate=True), 1, args.reps)
        approx.update({"rows": n, "rows_per_s": n / approx["median_s"], "output_bytes": n * (F + 1) * 4,
                       "output_GB_per_s": n * (F + 1) * 4 / approx["median_s"] / 1e9,
                       "vs_predict_step": approx["median_s"] / pred["median_s"]})
        res["predict_step_c360"] = pred
        res["approx_c360"] = approx
        print("approx_c360", json.dumps(approx), "predict", json.dumps(pred), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
