"""Timing of the selected-gridcells calls (OHXSelectCellsDevice, OHXGatherCellsDevice, OHXScatterCellsDevice) on the
benchmark's C360 L72 fields and synthetic OH booster (100 trees, depth <= 18, as bench.py builds it).  Device events
around each call after a warm-up, median of --reps (at least 5); the two end-to-end pipelines by a host clock around
work that ends in a device synchronise.  Writes one JSON document (default profiles/r10_cells_timing.json).

Reports:
  select_troposphere   PL_MOD > TROPP over the whole grid (a 3-D, b 2-D): cells found, time, GB/s on the bytes the two
                       passes read and the indices written;
  gather_4096, gather_1000000   the first 4 096 / 1 000 000 selected cells at 27 fields, GB/s on the bytes written;
  scatter_1000000      one column of the 1 000 000 cells' rows scattered back;
  column_pipeline      exact contributions of one column of 72 cells: select -> gather -> matrix over device memory ->
                       OHXBoosterPredictContribsDevice -> 28 scatters into arrays the caller holds, beside the same
                       with the row matrix built on the host from host copies of the fields and uploaded, and the
                       contributions downloaded."""
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
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "reps": reps}


def host_clock(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_cells_timing.json"))
    ap.add_argument("--grid", default="C360")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert args.reps >= 5
    assert torch.cuda.is_available(), "cells_timing needs the MI355X"
    torch.cuda.set_device(0)
    grid = synth.GRIDS[args.grid]
    im, jm, km = grid
    plane, total = im * jm, im * jm * km
    F = synth.NFEAT
    fields = []
    for f in range(F):
        t = torch.empty(plane * (1 if synth.IS2D[f] else km), dtype=torch.float32, device="cuda")
        synth.field_device(grid, f, t)
        fields.append(t)
    tropp = torch.empty(plane, dtype=torch.float32, device="cuda")
    synth.field_device(grid, -1, tropp)
    fp = [t.data_ptr() for t in fields]
    pl = fields[synth.PL_FEATURE]
    res = {"grid": list(grid), "gridcells": total}

    # ---- the troposphere selection over the whole grid ----
    cells = torch.empty(total, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    blocks, chunk = synth.cells_plan(total)[:2]

    def select():
        capi.select_cells_device(im, jm, km, None, pl.data_ptr(), False, tropp.data_ptr(), True, 0.0,
                                 cells.data_ptr(), total, count.data_ptr(), status.data_ptr())
    r = time_calls(select, 2, args.reps)
    nsel = int(count.item())
    # both passes read a and b at every cell (b, 2-D, from cache after the first level); the indices are written once
    moved = 2 * total * 4 * 2 + nsel * 8
    r.update({"selected": nsel, "status": int(status.item()), "blocks": blocks, "cells_per_block": chunk,
              "bytes": moved, "GB_per_s": moved / r["median_s"] / 1e9, "gridcells_per_s": total / r["median_s"]})
    res["select_troposphere"] = r
    print("select_troposphere", json.dumps(r), flush=True)

    # ---- gather ----
    for n in (4096, 1000000):
        n = min(n, nsel)
        rows = torch.empty((n, F), dtype=torch.float32, device="cuda")

        def gather():
            capi.gather_cells_device(fp, synth.IS2D, synth.PL_FEATURE, im, jm, km, cells.data_ptr(), n, rows.data_ptr(),
                                     status.data_ptr())
        r = time_calls(gather, 2, args.reps)
        r.update({"cells": n, "fields": F, "bytes_written": n * F * 4, "GB_per_s_written": n * F * 4 / r["median_s"] / 1e9,
                  "cells_per_s": n / r["median_s"], "status": int(status.item())})
        res[f"gather_{n}"] = r
        print(f"gather_{n}", json.dumps(r), flush=True)
    out3d = torch.zeros(total, dtype=torch.float32, device="cuda")

    def scatter():
        capi.scatter_cells_device(rows.data_ptr(), F, 3, cells.data_ptr(), n, out3d.data_ptr(), im, jm, km,
                                  status.data_ptr())
    r = time_calls(scatter, 2, args.reps)
    r.update({"cells": n, "cells_per_s": n / r["median_s"], "status": int(status.item())})
    res[f"scatter_{n}"] = r
    print(f"scatter_{n}", json.dumps(r), flush=True)
    del rows, out3d, cells
    torch.cuda.empty_cache()

    # ---- exact contributions of one column, end to end ----
    model = synth.make_model()
    b = capi.Booster(model_buffer=model.image)
    ic, jc = im // 3, jm // 2
    box = (ic, ic, jc, jc, 1, km)

    outs = [torch.zeros(total, dtype=torch.float32, device="cuda") for _ in range(F + 1)]     # the caller's arrays

    def device_pipeline():
        c, phi = b.explain_cells(fields, synth.IS2D, synth.PL_FEATURE, im, jm, km, synth.XX_MISS, box=box,
                                 scatter=False)
        for f in range(F + 1):
            capi.scatter_cells_device(phi.data_ptr(), F + 1, f, c.data_ptr(), c.numel(), outs[f].data_ptr(), im, jm, km)
        return c, phi
    host_fields = [t.cpu().numpy() for t in fields]          # as a host model holds them; not timed

    def host_pipeline():
        col = np.arange(km, dtype=np.int64) * plane + (ic - 1) + im * (jc - 1)
        rows = np.empty((km, F), dtype=np.float32)
        for f in range(F):
            v = host_fields[f][col % plane] if synth.IS2D[f] else host_fields[f][col]
            rows[:, f] = v / np.float32(100) if f == synth.PL_FEATURE else v
        d_rows = torch.from_numpy(rows).cuda()
        d = capi.DMatrix(device_ptr=d_rows.data_ptr(), nrow=km, ncol=F, missing=synth.XX_MISS)
        phi = torch.empty((km, F + 1), dtype=torch.float32, device="cuda")
        b.predict_contribs_device(d, phi.data_ptr())
        got = phi.cpu().numpy()
        d.free()
        return col, got
    dev = host_clock(device_pipeline, 2, args.reps)
    host = host_clock(host_pipeline, 2, args.reps)
    cells_d, phi_d = device_pipeline()
    col, got = host_pipeline()
    torch.cuda.synchronize()
    same = bool(np.array_equal(cells_d.cpu().numpy(), col) and
                np.array_equal(phi_d.cpu().numpy().view(np.uint32), got.view(np.uint32)) and
                all(np.array_equal(outs[f][cells_d].cpu().numpy().view(np.uint32), got[:, f].view(np.uint32))
                    for f in range(F + 1)))
    res["column_pipeline"] = {"cells": km, "column": [ic, jc], "device": dev, "host_built_rows": host,
                              "bits_equal": same,
                              "model": {"trees": model.num_trees, "nodes": model.num_nodes, "max_depth": model.max_depth}}
    print("column_pipeline", json.dumps(res["column_pipeline"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
