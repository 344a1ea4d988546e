"""What a rows predict launches, branch by branch of the launch plan (docs/05_kernels.md, "The launch plan"), on the
smoke booster (20 trees, depth <= 18) and the C12 batch (62 208 rows).

Every kernel gives the same bits, so a parity test cannot see a batch that went the wrong way: this one asserts the
exact list the library names for the batch (Booster.kernel_symbols_for).  The strings are what the library answered
BEFORE the plan was written in one place (kernels.hip plan_rows) - literals, never recomputed - so that a change of a
launch rule shows up here as a diff of this table.  The margins (or leaf ids) must equal the `wide` kernel's bit for bit."""
import numpy as np
import pytest

from quickchem_amd import capi, synth

pytestmark = pytest.mark.gpu

GRID = synth.GRIDS["C12"]
N = GRID[0] * GRID[1] * GRID[2]

RING = "predict_rows_ring_kernel + predict_rows_tile_kernel<2,2,true,true> (only after a ring time-out)"
MISSING = " (rows with missing values)"
COMBINE = " + combine_leaves_kernel"

# id: (booster parameters, rows, grid hint given, option_mask, what the library names)
#   rows: "rows27" the C12 rows; "rows20" their first 20 columns; "missing" the C12 rows with 200 entries per million missing
BRANCHES = {
    "auto": ({}, "rows27", True, 0, "predict_rows_tile_kernel<2,2,false,true>" + COMBINE),
    "tree_split_off": ({"ohx_tree_split": "off"}, "rows27", True, 0, RING),
    "super1": ({"ohx_kernel": "super1"}, "rows27", True, 0, "predict_rows_tile_kernel<2,1,false,true>" + COMBINE),
    "super2": ({"ohx_kernel": "super2"}, "rows27", True, 0, "predict_rows_tile_kernel<2,2,false,true>" + COMBINE),
    "super3": ({"ohx_kernel": "super3"}, "rows27", True, 0, "predict_rows_tile_kernel<2,3,false,true>" + COMBINE),
    "super4": ({"ohx_kernel": "super4"}, "rows27", True, 0, "predict_rows_tile_kernel<2,4,false,true>" + COMBINE),
    "packed1": ({"ohx_kernel": "packed1"}, "rows27", True, 0, "predict_rows_tile_kernel<1,1,true,false>"),
    "packed2": ({"ohx_kernel": "packed2"}, "rows27", True, 0, "predict_rows_tile_kernel<1,2,true,false>"),
    "packed4": ({"ohx_kernel": "packed4"}, "rows27", True, 0, "predict_rows_tile_kernel<1,4,true,false>"),
    "wide": ({"ohx_kernel": "wide"}, "rows27", True, 0, "predict_rows_direct_kernel<false>"),
    "columns_20": ({}, "rows20", True, 0, "predict_rows_tile_kernel<2,2,false,true>" + COMBINE),
    "pred_leaf": ({}, "rows27", True, 16, "predict_rows_tile_kernel<2,2,false,true>" + COMBINE),   # (names the margin predict)
    "defer_missing_on": ({"ohx_defer_missing": "on"}, "missing", True, 0, "predict_rows_tile_kernel<2,2,false,true>" + COMBINE),
    # (the query does not run the clustering pass: it names the plan of the rows in their own order, while the predict,
    # whose rows come through the pass's permutation, takes the ring kernel)
    "cluster_on_no_grid": ({"ohx_cluster": "on"}, "rows27", False, 0, "predict_rows_tile_kernel<2,2,false,true>" + COMBINE),
    "brick_8x4x2": ({"ohx_brick": "8,4,2"}, "rows27", True, 0, "predict_rows_tile_kernel<2,2,false,true>" + COMBINE),
    # the branches a batch this small only takes with the trees not split over waves
    "super2_tile": ({"ohx_kernel": "super2", "ohx_tree_split": "off"}, "rows27", True, 0,
                    "predict_rows_tile_kernel<2,2,true,true>"),
    "super3_tile_no_tops": ({"ohx_kernel": "super3", "ohx_tree_split": "off", "ohx_tree_tops": "off"}, "rows27", True, 0,
                            "predict_rows_tile_kernel<2,3,true,false>"),
    "ring_deferred": ({"ohx_tree_split": "off", "ohx_defer_missing": "on"}, "missing", True, 0,
                      RING + " + predict_rows_tile_kernel<2,2,false,true>" + MISSING),
    "super4_tile_deferred": ({"ohx_kernel": "super4", "ohx_tree_split": "off", "ohx_defer_missing": "on"}, "missing", True, 0,
                             "predict_rows_tile_kernel<2,4,true,true> + predict_rows_tile_kernel<2,4,false,true>" + MISSING),
    "columns_20_tile": ({"ohx_tree_split": "off"}, "rows20", True, 0, "predict_rows_tile_kernel<2,2,false,true>"),
    "ring_no_grid": ({"ohx_tree_split": "off", "ohx_cluster": "off"}, "rows27", False, 0, RING),
}


@pytest.fixture(scope="module")
def plan_inputs():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    model = synth.make_model(num_trees=20, max_depth=18, sample_log2=16, min_leaf=2, grid=GRID)
    rows = torch.empty((N, synth.NFEAT), dtype=torch.float32, device="cuda")
    synth.rows_device(GRID, 0, N, rows)
    missing = rows.clone()
    synth.inject_missing_device(missing, 200)
    torch.cuda.synchronize()
    return model, {"rows27": rows, "rows20": rows[:, :20].contiguous(), "missing": missing}, {}


def run_branch(model, rows, params, hint, option_mask):
    """-> (what the library names for the batch, what the predict wrote)"""
    import torch
    b = capi.Booster(model_buffer=model.image)
    for name, value in params.items():
        b.set_param(name, value)
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=rows.shape[0], ncol=rows.shape[1], missing=synth.XX_MISS)
    d.set_grid(GRID[0], GRID[1], 0) if hint else d.set_grid(0, 0, 0)
    out = torch.zeros(N * (model.num_trees if option_mask & 16 else 1), dtype=torch.float32, device="cuda")
    b.predict_device(d, out.data_ptr(), option_mask=option_mask, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    b.check()
    assert b.ring_reruns() == 0
    symbols = b.kernel_symbols_for(d)
    d.free()
    b.free()
    return symbols, out.cpu().numpy()


@pytest.mark.parametrize("branch", list(BRANCHES))
def test_a_batch_goes_the_way_the_plan_names(plan_inputs, branch):
    model, inputs, wide = plan_inputs
    params, rows, hint, option_mask, want = BRANCHES[branch]
    if (rows, option_mask) not in wide:      # the wide kernel's answer, once per input
        wide[(rows, option_mask)] = run_branch(model, inputs[rows], {"ohx_kernel": "wide"}, hint, option_mask)[1]
    symbols, got = run_branch(model, inputs[rows], params, hint, option_mask)
    print(f"{branch}: {symbols}")
    assert symbols == want
    assert np.array_equal(got.view(np.uint32), wide[(rows, option_mask)].view(np.uint32))
