"""BASELINE.json's full sizes on the GPU, through size-independent properties (the oracle would
take minutes at these sizes): kernels of different design agree bit for bit, shards concatenate
to the whole, and a random sample is checked against the oracle."""
import os

import numpy as np
import pytest

from quickchem_amd import capi, synth
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def full_model():
    return synth.make_model()          # 100 trees, depth <= 18, 2**20-row sample


def _predict_dev(torch, booster, rows, kernel):
    booster.set_param("ohx_kernel", kernel)
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=rows.shape[0], ncol=27, missing=synth.XX_MISS)
    out = torch.empty(rows.shape[0], dtype=torch.float32, device="cuda")
    booster.predict_device(d, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    booster.check()
    d.free()
    return out


@pytest.mark.parametrize("gridname,shard", [("C48", None), ("C180", None), ("C360", 8)])
def test_full_size_properties(full_model, gridname, shard):
    import torch
    torch.cuda.set_device(0)
    grid = synth.GRIDS[gridname]
    n = grid[0] * grid[1] * grid[2]
    if shard:                               # C360: one of the 8 contiguous row shards (6 998 400 rows)
        n //= shard
    row0 = 3 * n if shard else 0
    rows = torch.empty((n, 27), dtype=torch.float32, device="cuda")
    synth.rows_device(grid, row0, n, rows)
    synth.inject_missing_device(rows, 100)                     # 1e-4 of the entries: -999.0 or NaN
    booster = capi.Booster(model_buffer=full_model.image)
    a = _predict_dev(torch, booster, rows, "auto")             # the shipped default (the ring kernel for this booster)
    b = _predict_dev(torch, booster, rows, "wide")             # different node format, no LDS tile, 1 chain
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for other in ("packed1", "packed4", "super1", "super4"):
        c = _predict_dev(torch, booster, rows, other)
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), other
    # shards concatenate to the whole (what the 8-GPU run relies on)
    cut = (n // 3) // 64 * 64 + 17
    parts = [_predict_dev(torch, booster, rows[:cut], "auto"), _predict_dev(torch, booster, rows[cut:], "auto")]
    assert torch.equal(torch.cat(parts).view(torch.int32), a.view(torch.int32))
    # permutation equivariance on a block
    perm = torch.randperm(100_000, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    sub = rows[:100_000][perm].contiguous()
    assert torch.equal(_predict_dev(torch, booster, sub, "auto").view(torch.int32), a[:100_000][perm].view(torch.int32))
    # a random sample against the oracle, on the very same bytes
    idx = torch.randint(0, n, (50_000,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    sample = rows[idx].cpu().numpy()
    want = helpers.oracle_predict(full_model.image, sample, synth.XX_MISS)
    assert np.array_equal(helpers.bits(a[idx].cpu().numpy()), helpers.bits(want))
    assert torch.isfinite(a).all() and -16 < float(a.min()) and float(a.max()) < -10


def _hinted_vs_unhinted(torch, model, grid, row0, n, how):
    """The shipped default (super-nodes, bricks from the grid hint or from the inferred level size) against the
    `wide` kernel on the same rows without any hint (64 consecutive rows per wave, another node format), plus
    50 000 random rows against the oracle."""
    rows = torch.empty((n, 27), dtype=torch.float32, device="cuda")
    synth.rows_device(grid, row0, n, rows)
    booster = capi.Booster(model_buffer=model.image)
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=n, ncol=27, missing=synth.XX_MISS)
    if how == "hint":
        d.set_grid(grid[0], grid[1], row0)
        assert d.grid() == (grid[0], grid[1], row0, False)
    elif how == "infer":
        assert d.infer_grid() is True
        assert d.grid() == (grid[0] * grid[1], 1, 0, True)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    booster.predict_device(d, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    booster.check()
    if how == "lazy":               # nobody described the rows: the first predict looked for the level size
        assert d.grid() == (grid[0] * grid[1], 1, 0, True)
    d.free()
    ref = _predict_dev(torch, capi.Booster(model_buffer=model.image), rows, "wide")
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    idx = torch.randint(0, n, (50_000,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    want = helpers.oracle_predict(model.image, rows[idx].cpu().numpy(), synth.XX_MISS)
    assert np.array_equal(helpers.bits(out[idx].cpu().numpy()), helpers.bits(want))
    return out


@pytest.mark.parametrize("how", ["hint", "infer", "lazy"])
def test_whole_c360_batch_with_the_default_tiling(full_model, how):
    """The headline workload exactly as bench.py times it: all 55 987 200 rows of C360 L72 in ONE DMatrix,
    4x4x4 bricks from OHXDMatrixSetGrid(360, 2160, 0) - 32-bit brick numbering, 874 800 tiles, four launches of
    the ring kernel (64 rounds of 256 x 16 tiles each; the tile kernel's train was 86 launches until round 3);
    with the level size inferred (8 cells x 8 levels per wave); and with nothing said at all
    ("lazy": OHXBoosterPredictDevice looks for the level size itself at the first predict)."""
    import torch
    torch.cuda.set_device(0)
    grid = synth.GRIDS["C360"]
    _hinted_vs_unhinted(torch, full_model, grid, 0, grid[0] * grid[1] * grid[2], how)


def test_whole_c360_batch_against_the_oracle_row_for_row(full_model):
    """The headline step, every one of its 55 987 200 margins against the CPU oracle, bit for bit (not a sample and
    not another kernel: VERDICT r2 weak #2).  The oracle takes the batch eight levels at a time (672 MB of rows per
    piece on the host) with the OpenMP threads the box gives it; about a minute."""
    import time
    import torch
    torch.cuda.set_device(0)
    grid = synth.GRIDS["C360"]
    plane, n = grid[0] * grid[1], grid[0] * grid[1] * grid[2]
    rows = torch.empty((n, 27), dtype=torch.float32, device="cuda")
    synth.rows_device(grid, 0, n, rows)
    booster = capi.Booster(model_buffer=full_model.image)
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=n, ncol=27, missing=synth.XX_MISS)
    d.set_grid(grid[0], grid[1], 0)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    booster.predict_device(d, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    booster.check()
    d.free()
    got = out.cpu().numpy()
    t0 = time.time()
    for k in range(0, grid[2], 8):
        a, z = k * plane, min(n, (k + 8) * plane)
        want = helpers.oracle_predict(full_model.image, rows[a:z].cpu().numpy(), synth.XX_MISS)
        bad = np.flatnonzero(helpers.bits(got[a:z]) != helpers.bits(want))
        assert bad.size == 0, (k, bad[:5] + a, got[a:z][bad[:5]], want[bad[:5]])
        print(f"levels {k}-{k + 7}: {z - a} margins equal the oracle's, {time.time() - t0:.0f} s", flush=True)


@pytest.mark.parametrize("grid", [(180, 1080, 72), (183, 541, 72)])
def test_oh_run1_at_c180_against_the_oracle(full_model, grid):
    """The call the GridComp shell makes every tick (OHXBoosterRun1: engineered features, k-slab, fused gather +
    walk in a train of launches, tropopause mask, unit conversion; OH_GridCompMod.F90:1444-1488,275-374,1557-1595) on a
    whole C180 L72 state with the 100-tree depth-18 booster, and on a grid no side of which is a multiple of the brick,
    every gridcell against the CPU restatement: NDWET and the masked cells bit for bit, OH within 3 ulp (10**x)."""
    st = helpers.run1_state(grid, seed=grid[0])
    lib = helpers.oracle_lib()
    ob = capi.Booster(model_buffer=full_model.image, lib=lib)
    want = ob.run1(st, dynamic_k_range=True)
    ob.free()
    b = capi.Booster(model_buffer=full_model.image)
    got = b.run1(st, dynamic_k_range=True)
    again = b.run1(st, dynamic_k_range=True)                   # second tick: parked buffers, the deferral's history
    b.free()
    assert (got["k1"], got["k2"]) == (want["k1"], want["k2"]) and got["k1"] > 1
    assert np.array_equal(helpers.bits(got["ndwet"]), helpers.bits(want["ndwet"]))
    k1 = got["k1"]
    assert not got["oh_boost"][:, :, :k1 - 1].any()
    assert helpers.ulp_diff(got["oh_boost"][:, :, k1 - 1:], want["oh_boost"][:, :, k1 - 1:]).max() <= 2
    pl = (st["ple_mod"][:, :, :-1] + st["ple_mod"][:, :, 1:]) * np.float32(0.5)
    above = ~(pl > st["tropp_mod"][:, :, None])
    assert np.array_equal(helpers.bits(got["oh"][above]), helpers.bits(want["oh"][above]))
    assert helpers.ulp_diff(got["oh"][~above], want["oh"][~above]).max() <= 3
    for name in ("oh", "oh_boost", "ndwet"):
        assert np.array_equal(helpers.bits(again[name]), helpers.bits(got[name])), name


def test_c720_l137_shard_starting_inside_a_level(full_model):
    """Config #5 with the hint and a ragged start: one eighth of C720 L137 whose first row is 12 345 cells into
    a level (row0 not a multiple of im*jm), so the first and last bricks overhang the row range."""
    import torch
    torch.cuda.set_device(0)
    grid = synth.GRIDS["C720L137"]
    n = grid[0] * grid[1] * grid[2] // 8
    _hinted_vs_unhinted(torch, full_model, grid, 5 * n + 12_345, n, "hint")


def test_c720_l137_shard_with_twelve_resident_boosters():
    """BASELINE.json config #5: one of the 8 row shards of C720 L137 (53 265 600 gridcells, 5.75 GB of
    features) with twelve monthly boosters resident in HBM at once (the reference keeps one booster per
    process and never reloads on month roll-over, OH_GridCompMod.F90:209,269; OH_instance_OH.rc:20)."""
    import torch
    torch.cuda.set_device(0)
    grid = synth.GRIDS["C720L137"]
    n = grid[0] * grid[1] * grid[2] // 8
    assert n == 53_265_600
    rows = torch.empty((n, 27), dtype=torch.float32, device="cuda")
    synth.rows_device(grid, 5 * n, n, rows)
    models = [synth.make_model(sample_log2=18, min_leaf=4, model_seed=synth.MODEL_SEED + 100 * m) for m in range(12)]
    boosters = [capi.Booster(model_buffer=m.image) for m in models]
    idx = torch.randint(0, n, (20_000,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    sample = rows[idx].cpu().numpy()
    first = None
    for month in (0, 6, 11, 0):
        out = _predict_dev(torch, boosters[month], rows, "auto")
        want = helpers.oracle_predict(models[month].image, sample, synth.XX_MISS)
        assert np.array_equal(helpers.bits(out[idx].cpu().numpy()), helpers.bits(want)), month
        if month == 0:
            if first is None:
                first = out.clone()
            else:
                assert torch.equal(first.view(torch.int32), out.view(torch.int32))   # other boosters did not disturb it
    # different months really are different models
    assert not torch.equal(first.view(torch.int32), _predict_dev(torch, boosters[6], rows, "auto").view(torch.int32))


def test_two_ranks_share_the_gpu_and_agree_with_one(tmp_path):
    """Rehearsal of the N > 1 path of bench.py on the one GPU of the box: two ranks (gloo; RCCL refuses two
    ranks on one device), each predicting its shard of C90 L72 in level-aligned pieces with its own grid
    offset, asynchronous all-gathers into place; rank 0 then predicts the whole batch in one untiled piece
    and the two fields must be bit-identical (`--verify`)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OHX_BENCH_SHARE_GPU="1", OHX_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    # started plainly, the way the driver starts every N: bench.py launches its two ranks itself
    plain = {k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    for extra in ([], ["--gather-chunks", "1"]):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"),
                            "--gpus", "2", "--grid", "C90", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0",
                            "--full"] + extra, capture_output=True, text=True, env=plain, timeout=900, cwd=root)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        assert len([ln for ln in r.stdout.splitlines() if ln.startswith("{")]) == 1
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["config"]["verified"] is True and line["n_gpus"] == 2 and line["config"]["grid_hint"] is True
        assert line["phases"]["even_shards"] is True and line["phases"]["gather_bytes_total"] == 4 * 90 * 540 * 72
        assert line["phases"]["predict_ms"] > 0 and len(line["distributed"]["ranks"]) == 2
        # (r5) the line explains itself: both ranks' numbers, the control loop without the gather, the priced plans
        ph = line["phases"]
        assert line["config"]["gather_via"] == "both" and len(ph["per_rank"]["step_ms"]) == 2
        assert len(ph["per_rank"]["predict_ms"]) == 2 and ph["per_rank"]["rows"] == [90 * 540 * 36] * 2
        assert ph["predict_only"]["step_ms"] > 0 and len(ph["predict_only"]["per_rank_step_ms"]) == 2
        assert ph["plan"]["prices"]["gather_bytes_per_s"] == 100e9 and sum(r["chosen"] for r in ph["plan"]["priced"]) == 1
        assert [r for r in ph["plan"]["priced"] if r["chosen"]][0]["sizes"] == ph["pieces"]
    # under torch.distributed.run (the other way to start it): ragged shards (an odd number of rows over two ranks:
    # the fixed-slot gather and its compaction), and the predict-only control that a scaling curve is split with
    for extra in (["--rows", "995327"], ["--gather", "none"]):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", "29578", os.path.join(root, "bench.py"),
                            "--gpus", "2", "--grid", "C48", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0",
                            "--full"] + extra, capture_output=True, text=True, env=env, timeout=900, cwd=root)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["config"]["verified"] is True and line["n_gpus"] == 2
        if extra[0] == "--rows":
            assert line["config"]["rows_total"] == 995327 and line["phases"]["even_shards"] is False
            assert line["config"]["rows_per_gpu"] == 497664                      # rank 0 holds the odd row
        else:
            assert line["config"]["gather_pieces"] == 0 and line["config"]["gather_via"] == "none"


def test_bench_over_rccl_with_one_rank():
    """What the driver's N > 1 runs execute, as far as one GPU can: bench.py with the RCCL process group of ONE rank
    (OHX_BENCH_FORCE_DIST=1) - the chunked all-gather through torch.distributed, the C ABI's OHXAllGatherOH, and the
    predict-only control; the line carries the phases and the record of who ran where over which RCCL."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OHX_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29581")
    for gather in ("both", "torch", "native", "none"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--grid", "C90", "--steps", "2",
                            "--warmup", "1", "--cpu-seconds", "0", "--full", "--gather", gather, "--gather-gbps", "60"],
                           capture_output=True, text=True, env=env, timeout=900, cwd=root)
        assert r.returncode == 0, (gather, r.stdout[-1500:], r.stderr[-3000:])
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["config"]["verified"] is True and line["config"]["gather_via"] == gather
        d = line["distributed"]
        assert d["backend"] == "nccl" and d["world_size"] == 1 and len(d["ranks"]) == 1
        assert d["rccl_version"] and d["rccl_version"] >= 20000
        ph = line["phases"]
        assert ph["predict_ms"] > 0 and ph["gather_bytes_total"] == 4 * 90 * 540 * 72
        assert line["config"]["gather_pieces"] == (0 if gather == "none" else len(ph["pieces"]))
        assert line["config"]["planner_prices"]["gather_bytes_per_s"] == 60e9 and ("predict_only" in ph) == (gather == "both")


def test_bench_dumps_what_its_timed_steps_computed(tmp_path):
    """bench.py --dump-outputs: the margins of the last timed step are the oracle's, row for row; they do not depend on
    --steps, which the line reports back with ms_per_step; the fused path dumps its OH field."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    small = ["--grid", "C48", "--trees", "20", "--depth", "10", "--sample-log2", "15", "--cpu-seconds", "0", "--no-pcie"]

    def bench(steps, out, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", "1", "--dump-outputs", str(out), *small, *extra],
                           capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        return line

    bench(1, tmp_path / "one")
    bench(3, tmp_path / "three")
    assert os.listdir(tmp_path / "one") == ["margins.npy"]
    got = np.load(tmp_path / "one" / "margins.npy")
    assert got.dtype == np.float32 and got.shape == (48 * 288 * 72,)
    assert np.array_equal(helpers.bits(got), helpers.bits(np.load(tmp_path / "three" / "margins.npy")))
    model = synth.make_model(num_trees=20, max_depth=10, sample_log2=15)
    want = helpers.oracle_predict(model.image, synth.rows_cpu(synth.GRIDS["C48"], 0, got.shape[0]), synth.XX_MISS)
    assert np.array_equal(helpers.bits(got), helpers.bits(want))
    bench(2, tmp_path / "fields", "--path", "fields")
    oh = np.load(tmp_path / "fields" / "oh.npy")
    assert oh.dtype == np.float32 and oh.shape == (48 * 288 * 72,) and np.all(oh > 0)


def test_native_all_gather_entry_points_on_one_rank():
    """include/ohxgb.h part 4 with the one GPU of the box: RCCL is found and loaded by libohxgb.so itself, a
    communicator of one rank is built from a unique id, and OHXAllGatherOH puts the shard at its rows - out of place
    and in place.  (More than one rank needs more than one GPU: RCCL refuses two ranks on a device; the
    sharding rule itself is covered on the CPU by tests/test_distributed_gloo.py.)"""
    import torch
    torch.cuda.set_device(0)
    uid = capi.Communicator.unique_id()
    assert len(uid) == capi.UNIQUE_ID_BYTES and any(uid)
    comm = capi.Communicator(uid, 1, 0)
    n = 1_000_003
    shard = torch.arange(n, dtype=torch.float32, device="cuda")
    full = torch.zeros(n, dtype=torch.float32, device="cuda")
    comm.all_gather_oh(shard.data_ptr(), n, n, full.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(full, shard)
    comm.all_gather_oh(full.data_ptr(), n, n, full.data_ptr())          # in place
    torch.cuda.synchronize()
    assert torch.equal(full, shard)
    # the direct exchange (every shard to every peer as one group of sends and receives): with one rank its own
    # rows are a device copy and the group is empty - the code path of ragged shards
    # (the route is fixed when the communicator is made: a setenv between two calls cannot split the ranks)
    os.environ["OHX_ALLGATHER"] = "pairs"
    try:
        pairs = capi.Communicator(capi.Communicator.unique_id(), 1, 0)
    finally:
        del os.environ["OHX_ALLGATHER"]
    full.zero_()
    pairs.all_gather_oh(shard.data_ptr(), n, n, full.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(full, shard)
    pairs.free()
    assert capi.Communicator.rccl_version() >= 20000                     # ncclGetVersion of the library that was loaded
    with pytest.raises(capi.OhxError, match="holds 5 rows"):
        comm.all_gather_oh(shard.data_ptr(), 5, n, full.data_ptr())
    with pytest.raises(capi.OhxError, match="rank < nranks"):
        capi.Communicator(uid, 2, 2)
    comm.free()
    with pytest.raises(capi.OhxError, match="invalid or has been freed"):
        capi.check(comm.lib, comm.lib.OHXAllGatherOH(0xDEAD0, None, 0, 0, None, None))
