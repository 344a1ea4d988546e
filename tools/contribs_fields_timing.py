"""Timing of per-feature contributions from the fields (OHXBoosterPredictContribsFieldsDevice: 27 fields in HBM ->
28 feature-major (im,jm,km) arrays) on the benchmark's synthetic OH booster (100 trees, depth <= 18, grown on 2**20
cells, as bench.py builds it).  Device events around each call after a warm-up, median of --reps; writes one JSON
document (default profiles/r07_contribs_fields_timing.json).

Reports:
  approx_c360        approximate mode on the whole C360 L72 grid, beside the rows-form device call
                     (OHXBoosterPredictContribsDevice, [n][28] row-major) on the same gridcells in the same process,
                     and whether the two agree bit for bit on every gridcell and feature;
  approx_rank_block  approximate mode on one 48 x 24 x 72 rank block (the cost of a per-tick export);
  exact_rank_block   exact mode on the same block (--skip-exact leaves it out)."""
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


def time_calls(fn, warmup, reps, inner=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / 1e3 / inner)
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "reps": reps, "calls_per_rep": inner}


def device_fields(grid):
    F = synth.NFEAT
    out = []
    for f in range(F):
        n = grid[0] * grid[1] * (1 if synth.IS2D[f] else grid[2])
        t = torch.empty(n, dtype=torch.float32, device="cuda")
        synth.field_device(grid, f, t)
        out.append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_contribs_fields_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-exact", action="store_true")
    ap.add_argument("--skip-c360", action="store_true")
    ap.add_argument("--skip-rank-block", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "contribs_fields_timing needs the MI355X"
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    model = synth.make_model()
    res = {"model": {"trees": model.num_trees, "nodes": model.num_nodes, "leaves": model.num_leaves,
                     "max_depth": model.max_depth}, "model_seconds": time.perf_counter() - t0}
    b = capi.Booster(model_buffer=model.image)
    F = synth.NFEAT

    def fields_case(grid, approximate, warmup, inner):
        n = grid[0] * grid[1] * grid[2]
        fields = device_fields(grid)
        outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(F + 1)]
        fp, op = [t.data_ptr() for t in fields], [t.data_ptr() for t in outs]

        def call():
            b.predict_contribs_fields_device(fp, synth.IS2D, synth.PL_FEATURE, *grid, 1, grid[2], synth.XX_MISS, op,
                                             approximate=approximate)
        r = time_calls(call, warmup, args.reps, inner)
        r.update({"gridcells": n, "gridcells_per_s": n / r["median_s"], "output_bytes": n * (F + 1) * 4,
                  "output_GB_per_s": n * (F + 1) * 4 / r["median_s"] / 1e9})
        return r, fields, outs

    if not args.skip_c360:
        grid = synth.GRIDS["C360"]
        n = grid[0] * grid[1] * grid[2]
        r, fields, outs = fields_case(grid, True, 1, 1)
        del fields
        torch.cuda.empty_cache()
        # the rows form on the same gridcells, same process
        rows = torch.empty((n, F), dtype=torch.float32, device="cuda")
        synth.rows_device(grid, 0, n, rows)
        d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=n, ncol=F, missing=synth.XX_MISS)
        d.set_grid(grid[0], grid[1], 0)
        out_rows = torch.empty((n, F + 1), dtype=torch.float32, device="cuda")
        rr = time_calls(lambda: b.predict_contribs_device(d, out_rows.data_ptr(), approximate=True), 1, args.reps)
        rr.update({"rows": n, "output_GB_per_s": n * (F + 1) * 4 / rr["median_s"] / 1e9})
        r["rows_form_device"] = rr
        r["fields_over_rows"] = r["median_s"] / rr["median_s"]
        # Bit for bit on every gridcell: the synthetic PL field (Pa) is the rows' hPa value * 100, and / 100 does not
        # always give it back, so the fields for this check are the rows' own columns (2-D ones: the first level),
        # with no PL division
        plane = grid[0] * grid[1]
        cols = [(rows[:plane, f] if synth.IS2D[f] else rows[:, f]).contiguous() for f in range(F)]
        b.predict_contribs_fields_device([t.data_ptr() for t in cols], synth.IS2D, -1, *grid, 1, grid[2],
                                         synth.XX_MISS, [t.data_ptr() for t in outs], approximate=True)
        torch.cuda.synchronize()
        same = all(torch.equal(out_rows[:, f].contiguous().view(torch.int32), outs[f].view(torch.int32))
                   for f in range(F + 1))
        r["bits_equal_rows_form"] = bool(same)
        del cols
        d.free()
        del rows, out_rows, outs
        torch.cuda.empty_cache()
        res["approx_c360"] = r
        print("approx_c360", json.dumps(r), flush=True)
    block = (48, 24, 72)
    if not args.skip_rank_block:
        r, _, _ = fields_case(block, True, 3, 20)
        res["approx_rank_block_48x24x72"] = r
        print("approx_rank_block", json.dumps(r), flush=True)
    if not args.skip_exact:
        r, _, _ = fields_case(block, False, 1, 1)
        res["exact_rank_block_48x24x72"] = r
        print("exact_rank_block", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
