"""Timing of SHAP interaction values (OHXBoosterPredictInteractionsDevice) on the benchmark's synthetic OH booster
(100 trees, depth <= 18, as bench.py builds it).  Device events around each call after a warm-up, median of the
repetitions; writes one JSON document (default profiles/interactions_timing.json).

Reports: exact interactions on 64 and 4 096 rows, approximate interactions on a 48 x 24 x 72 rank block, the
feature-path index's size, and the least time exact mode's recurrences could take on the chip at the VALU-instruction
counts per element step of the contributions kernel (docs/12_contributions.md 12.3: 5 per extend step, 8 per
unwound step; interactions.hip runs the same recurrences).  For every path of d distinct features and every element c
of it, the path without c takes (d-1)d/2 extend steps and (d-1)^2 unwound steps; the contributions pass that gives phi
adds d(d+1)/2 and d^2.  `--resource-report` adds the compiler's kernel-resource-usage remarks (a text file)."""
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

VALU_WAVE_ISSUES_PER_S = 256 * 4 * 2.4e9 / 2     # MI355X: 256 CUs x 4 SIMDs, a wave64 VALU op in 2 cycles at 2.4 GHz


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interactions_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--extend-valu", type=float, default=5.0)
    ap.add_argument("--unwind-valu", type=float, default=8.0)
    ap.add_argument("--resource-report", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "interactions_timing needs the MI355X"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    model = synth.make_model()
    st = synth.interactions_table_stats(model.image)
    res = {"model": {"trees": model.num_trees, "nodes": model.num_nodes, "leaves": model.num_leaves},
           "index": st, "model_seconds": time.perf_counter() - t0}
    if args.resource_report:
        with open(args.resource_report) as f:
            res["kernel_resource_usage"] = f.read().splitlines()
    s1, s2, s3 = st["sum_d"], st["sum_d2"], st["sum_d3"]
    inter_wave = args.extend_valu * (s3 - s2) / 2 + args.unwind_valu * (s3 - 2 * s2 + s1)
    phi_wave = args.extend_valu * (s2 + s1) / 2 + args.unwind_valu * s2
    res["valu_per_tile"] = {"interactions": inter_wave, "contributions_pass": phi_wave,
                            "ratio": inter_wave / phi_wave}
    b = capi.Booster(model_buffer=model.image)
    F = synth.NFEAT

    def case(name, grid, nrow, approximate):
        rows = torch.empty((nrow, F), dtype=torch.float32, device="cuda")
        synth.rows_device(grid, 0, nrow, rows)
        out = torch.empty((nrow, F + 1, F + 1), dtype=torch.float32, device="cuda")
        d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=nrow, ncol=F, missing=synth.XX_MISS)
        t = time.perf_counter()
        b.predict_interactions_device(d, out.data_ptr(), approximate=approximate)   # the warm-up; builds the tables
        torch.cuda.synchronize()
        first = time.perf_counter() - t
        r = time_calls(lambda: b.predict_interactions_device(d, out.data_ptr(), approximate=approximate), 0, args.reps)
        r.update({"rows": nrow, "rows_per_s": nrow / r["median_s"], "first_call_s": first,
                  "chip_us_per_row": r["median_s"] / nrow * 1e6,
                  "plan": None if approximate else synth.interactions_plan(nrow, F, model.num_trees)})
        margin = torch.empty(nrow, dtype=torch.float32, device="cuda")
        b.predict_device(d, margin.data_ptr(), option_mask=1)
        torch.cuda.synchronize()
        o = out.double()
        err = (o.sum(dim=(1, 2)) - margin.double()).abs() / (1.0 + o.abs().sum(dim=(1, 2)))
        r["local_accuracy_max_rel"] = float(err.max())
        if not approximate:
            bound = -(-nrow // 64) * (inter_wave + phi_wave) / VALU_WAVE_ISSUES_PER_S
            r.update({"valu_bound_s": bound, "share_of_valu_bound": bound / r["median_s"]})
        d.free()
        res[name] = r
        print(name, json.dumps(r), flush=True)

    case("exact_64_rows", synth.GRIDS["C12"], 64, False)
    case("exact_4096_rows", synth.GRIDS["C12"], 4096, False)
    case("approx_rank_block_48x24x72", (48, 24, 72), 48 * 24 * 72, True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
