"""Timing of OHXBoosterBoostTreesDevice on the benchmark's synthetic OH booster (100 trees, depth <= 18, as bench.py
builds it) and the C360 L72 rows resident in HBM.  Labels = the margins of a booster of the same recipe grown from
another seed, as tools/refit_timing.py takes them.  Run by hand on an MI355X; writes one JSON document (default
profiles/boost_timing.json).

The cuts come from OHXQuantileCuts on a sample of `--sample` rows copied to the host (`--cuts host`), from
OHXDMatrixQuantileCuts on the same evenly strided rows where they lie (`--cuts device`), or from both, each timed and
the two compared (`--cuts both`, the default); `--cuts-full` also times the device call on every row (row_step = 1).
The trees are grown over the host's cuts where they were made, else over the device's.  The whole boost call is timed
from the host (it waits at its end): a fresh booster's first call, which also allocates the state's buffers, and the second call
of the same shape on one booster, which finds them, for 1 round and for `--rounds` rounds at `--max-depth`.  The one-off cost
(binning, the initial margin, the allocations' reuse) is what a 1-round call takes beyond one round's share of the long
call.  The RMSE against the labels is taken before the call, after a refit, and after the refit plus `--rounds` rounds.

The kernels' own times - the binning, and per level the histogram, split and partition kernels - come from a second
run of this script under a kernel trace with --reps 1 --rounds 1 (docs/18_boost_trees.md 18.4 says how).

`--holdout K` times OHXBoosterBoostTreesEvalDevice instead (docs/20_boost_eval.md): every K-th row is held out, the others
are the training rows (both gathered once into matrices of their own in HBM).  The plain boost call on the training rows,
the call with patience 0 and the call with `--patience` are each timed as the median of `--reps` calls after a first one,
on fresh boosters, `--rounds` rounds.  The per-round RMSE of both sets as the call returns it is written beside the one
this script computes itself, in torch from margin predicts, before the call and after its last kept tree.

`--weights ones|random` times OHXBoosterBoostTreesWeightedDevice (docs/21_row_weights.md) wherever `--weights none` (the
default) times the plain call, with a weight of 1.0 a row or weights uniform in [0, 4) in HBM, no held-out set and
min_child_weight 1; the timings stand under the same keys, so three runs that differ in `--weights` alone compare.

`--subsample S` and / or `--colsample C` time OHXBoosterBoostTreesSampledDevice (docs/22_sampling.md) in the same place,
with `--seed` and the weights `--weights` names (none: a NULL pointer); the plan written is the one over the n_sel features
a tree sees.  `--subsample 1 --colsample 1` is the sampled entry point on the weighted path.

`--deep` times OHXBoosterBoostTreesDeepDevice (docs/23_deep_trees.md) in the same place, with any `--max-depth` up to 18
and the weights `--weights` names (none: a NULL pointer); the plan written is plan_grow_deep's.  `--deep-only` skips the
first-call timing and the refit, for a run under a kernel trace or a quick look at one depth.

`--deep` with `--subsample S` and / or `--colsample C` times OHXBoosterBoostTreesDeepSampledDevice
(docs/24_deep_sampled.md) in the same place, with `--seed`; the plan written is plan_grow_deep_sampled's over the n_sel
features a tree sees.  Without the two fractions `--deep` does what it did.

`--objective pseudohuber` (with `--huber-slope`) and `--pairs on` set "ohx_objective", "ohx_huber_slope" and
"ohx_grow_pairs" on every booster that is timed (docs/26_objectives.md): the calls with row weights, `--weights`,
`--subsample` / `--colsample` or `--deep`, then go through the pair kernels.  Three runs that differ in these alone compare
the inline path, squared error on pairs and pseudo-Huber.  The refit at the end is a squared-error step and is left out
under pseudohuber.  `--objective quantile` (with `--quantile-alpha`) sets "ohx_objective" and "ohx_quantile_alpha"
(docs/32_quantile_objective.md): the calls with row weights at depth <= 8, never `--deep`; `--eval-metric quantile` reads the
same alpha.

`--monotone "(1,0,-1)"` sets "ohx_monotone_constraints" on every booster that is timed (docs/28_monotone_constraints.md): the
calls with row weights then take the constrained split kernels over the pair path.  Against a run with `--pairs on
--max-delta-step 0.5` - the same pair and histogram kernels and the same gain form - the difference is the split kernels
and the trees they choose; the node counts stand beside the times.

`--interaction-constraints "[[0,1,2],[3,4]]"` sets "ohx_interaction_constraints" on every booster that is timed
(docs/35_interaction_constraints.md): the calls with row weights then take the split kernels of grow_interact.hip over the
pair path.  Against a run with `--pairs on` - the same pair and histogram kernels - the difference is the split kernels and
the trees they choose; the node counts stand beside the times.

`--colsample-bylevel L` and `--colsample-bynode N` set "ohx_colsample_bylevel" and "ohx_colsample_bynode" on every booster
that is timed (docs/29_colsample_level_node.md), with `--subsample` / `--colsample`: the sampled calls then add the columns
of a level's own list and take the column-sampled split kernels over the pair path.  Against a run with `--pairs on` and
the same `--subsample` / `--colsample` the difference is the columns the histogram kernels add, the split kernels and the
trees they choose.  Left out, neither parameter is set."""
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


def holdout(args, model, rows, labels, n, F, stream):
    """Every K-th row held out: the plain call on the training rows against the call with a held-out set."""
    k = args.holdout
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[::k] = False
    xt, yt = rows[keep].contiguous(), labels[keep].contiguous()
    xe, ye = rows[::k].contiguous(), labels[::k].contiguous()
    del keep
    torch.cuda.synchronize()
    nt, ne = xt.shape[0], xe.shape[0]
    dt = capi.DMatrix(device_ptr=xt.data_ptr(), nrow=nt, ncol=F, missing=synth.XX_MISS)
    de = capi.DMatrix(device_ptr=xe.data_ptr(), nrow=ne, ncol=F, missing=synth.XX_MISS)
    cuts = dt.quantile_cuts(max(1, nt // args.sample), args.max_bins, stream=stream)
    pk = dict(rounds=args.rounds, max_depth=args.max_depth, eta=args.eta, reg_lambda=args.reg_lambda, stream=stream)

    def own_rmse(b, dm, x, y):
        out = torch.empty(x.shape[0], dtype=torch.float32, device="cuda")
        b.predict_device(dm, out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        b.check()
        return float(torch.sqrt(torch.mean((out.double() - y.double()) ** 2)).item())

    def timed(call):
        """-> (seconds of the calls after a first one, each on a fresh booster; the last result; its booster)."""
        times, last, b = [], None, None
        for _ in range(args.reps + 1):
            if b is not None:
                b.free()
            b = capi.Booster(model_buffer=model.image)
            torch.cuda.synchronize()
            t = time.perf_counter()
            last = call(b)
            times.append(time.perf_counter() - t)
        return times[1:] if args.reps else times, last, b

    def summary(times):
        return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times))}

    out = {"every": k, "training_rows": nt, "held_out_rows": ne, "rounds": args.rounds, "cut_values": int(cuts[0][-1]),
           "eval_plan": {"training": synth.grow_eval_plan(nt, torch.cuda.get_device_properties(0).multi_processor_count),
                         "held_out": synth.grow_eval_plan(ne, torch.cuda.get_device_properties(0).multi_processor_count)}}
    times, nodes, b = timed(lambda b: b.boost_trees_device(dt, yt.data_ptr(), nt, cuts, **pk))
    out["plain"] = dict(summary(times), nodes_added=nodes)
    b.free()
    for name, patience in (("patience_0", 0), (f"patience_{args.patience}", args.patience)):
        b0 = capi.Booster(model_buffer=model.image)
        before = None if args.skip_rmse else (own_rmse(b0, dt, xt, yt), own_rmse(b0, de, xe, ye))
        b0.free()
        times, r, b = timed(lambda b: b.boost_trees_eval_device(dt, yt.data_ptr(), nt, cuts, eval_set=(de, ye.data_ptr(), ne),
                                                                patience=patience, **pk))
        doc = dict(summary(times), rounds_run=r["rounds_run"], best_round=r["best_round"], nodes_added=r["nodes_added"],
                   train_rmse=r["train_rmse"].tolist(), eval_rmse=r["eval_rmse"].tolist(),
                   over_plain_s=float(np.median(times)) - out["plain"]["median_s"])
        if before is not None:
            # this script's own figures: the forest as loaded, and the forest the call left (its kept trees)
            kept = r["best_round"] if patience >= 1 else r["rounds_run"]
            doc["own_rmse"] = {"round_0": {"train": before[0], "eval": before[1]},
                               f"round_{kept}": {"train": own_rmse(b, dt, xt, yt), "eval": own_rmse(b, de, xe, ye)}}
        b.free()
        out[name] = doc
    for m in (dt, de):
        m.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boost_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid", default="C360", help="a name of synth.GRIDS")
    ap.add_argument("--label-seed", type=int, default=synth.MODEL_SEED + 1)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--eta", type=float, default=0.3)
    ap.add_argument("--reg-lambda", type=float, default=1.0)
    ap.add_argument("--max-bins", type=int, default=255)
    ap.add_argument("--sample", type=int, default=1 << 20)
    ap.add_argument("--cuts", choices=("host", "device", "both"), default="both")
    ap.add_argument("--cuts-full", action="store_true", help="also time the device cuts on every row (row_step = 1)")
    ap.add_argument("--skip-rmse", action="store_true", help="time only (a run under a kernel trace)")
    ap.add_argument("--holdout", type=int, default=0, help="hold out every K-th row and time the call with a held-out set")
    ap.add_argument("--patience", type=int, default=3, help="with --holdout: the patience of the early-stopping call")
    ap.add_argument("--weights", choices=("none", "ones", "random"), default="none",
                    help="ones / random: time OHXBoosterBoostTreesWeightedDevice in place of the plain call")
    ap.add_argument("--subsample", type=float, default=None, help="time OHXBoosterBoostTreesSampledDevice with this fraction of the rows a tree")
    ap.add_argument("--colsample", type=float, default=None, help="... and this fraction of the features a tree (colsample_bytree)")
    ap.add_argument("--seed", type=int, default=0, help="the seed of the sampled call's draws")
    ap.add_argument("--deep", action="store_true", help="time OHXBoosterBoostTreesDeepDevice (with --subsample / --colsample: ...DeepSampledDevice): --max-depth up to 18")
    ap.add_argument("--deep-only", action="store_true", help="with --deep: one call a round count on a fresh booster, no refit")
    ap.add_argument("--objective", choices=("squarederror", "pseudohuber", "quantile"), default="squarederror", help="ohx_objective of the timed boosters")
    ap.add_argument("--huber-slope", type=float, default=1.0, help="ohx_huber_slope of the timed boosters")
    ap.add_argument("--quantile-alpha", type=float, default=0.5, help="ohx_quantile_alpha of the timed boosters")
    ap.add_argument("--pairs", choices=("auto", "on"), default="auto", help="ohx_grow_pairs of the timed boosters")
    ap.add_argument("--reg-alpha", type=float, default=0.0, help="ohx_reg_alpha of the timed boosters")
    ap.add_argument("--max-delta-step", type=float, default=0.0, help="ohx_max_delta_step of the timed boosters")
    ap.add_argument("--eval-metric", choices=("rmse", "mae", "pseudohuber", "quantile"), default="rmse", help="ohx_eval_metric of the timed boosters")
    ap.add_argument("--monotone", default=None, help="ohx_monotone_constraints of the timed boosters, as the parameter is written: \"(1,0,-1)\"")
    ap.add_argument("--interaction-constraints", default=None,
                    help="ohx_interaction_constraints of the timed boosters, as the parameter is written: \"[[0,1,2],[3,4]]\"")
    ap.add_argument("--colsample-bylevel", type=float, default=None, help="ohx_colsample_bylevel of the timed boosters (with --subsample / --colsample)")
    ap.add_argument("--colsample-bynode", type=float, default=None, help="ohx_colsample_bynode of the timed boosters (with --subsample / --colsample)")
    args = ap.parse_args()
    sampled = args.subsample is not None or args.colsample is not None
    if sampled:
        args.subsample = 1.0 if args.subsample is None else args.subsample
        args.colsample = 1.0 if args.colsample is None else args.colsample
    if sampled and args.holdout:
        ap.error("--subsample / --colsample time the call without a held-out set: leave --holdout out")
    if args.deep and args.holdout:
        ap.error("--deep times the call without a held-out set: leave --holdout out")
    if args.weights != "none" and args.holdout:
        ap.error("--weights times the call without a held-out set: leave --holdout out")
    if (args.colsample_bylevel is not None or args.colsample_bynode is not None) and not sampled:
        ap.error("--colsample-bylevel / --colsample-bynode act on the calls that carry a seed: give --subsample / --colsample")
    regularised = args.reg_alpha != 0.0 or args.max_delta_step != 0.0 or args.eval_metric != "rmse"
    if (args.objective != "squarederror" or args.pairs != "auto" or regularised or args.monotone is not None or
            args.interaction_constraints is not None) and (args.holdout or not (sampled or args.deep or args.weights != "none")):
        ap.error("--objective / --pairs / --reg-alpha / --max-delta-step / --eval-metric / --monotone / --interaction-constraints time a call with row weights: give --weights, --subsample / --colsample or --deep, and no --holdout")
    assert torch.cuda.is_available(), "boost_timing needs the MI355X"
    torch.cuda.set_device(0)
    model = synth.make_model()
    teacher = synth.make_model(model_seed=args.label_seed)
    F = synth.NFEAT
    grid = synth.GRIDS[args.grid]
    n = grid[0] * grid[1] * grid[2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = torch.empty((n, F), dtype=torch.float32, device="cuda")
    synth.rows_device(grid, 0, n, rows)
    stream = torch.cuda.current_stream().cuda_stream
    d = capi.DMatrix(device_ptr=rows.data_ptr(), nrow=n, ncol=F, missing=synth.XX_MISS)
    d.set_grid(grid[0], grid[1], 0)
    # the cuts: quantiles of an evenly strided sample of the rows
    step = max(1, n // args.sample)
    res = {"model": {"trees": model.num_trees, "nodes": model.num_nodes, "max_depth": model.max_depth}, "rows": n,
           "max_depth": args.max_depth, "eta": args.eta, "reg_lambda": args.reg_lambda, "reps": args.reps,
           "row_step": step, "sample_rows": -(-n // step), "cuts_plan": synth.cuts_plan(n, step, F, cus)}
    cuts = None
    if args.cuts in ("host", "both"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sample = rows[::step].cpu().numpy()
        cuts = capi.quantile_cuts(sample, synth.XX_MISS, args.max_bins)
        res["cuts_host_seconds"] = time.perf_counter() - t0

    def device_cuts(row_step):
        """-> (the cuts, the seconds of a first call and of the `--reps` calls after it)."""
        times = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            c = d.quantile_cuts(row_step, args.max_bins, stream=stream)
            times.append(time.perf_counter() - t)
        return c, times

    if args.cuts in ("device", "both"):
        dcuts, times = device_cuts(step)
        res["cuts_device_first_call_seconds"] = times[0]
        res["cuts_device_seconds"] = float(np.median(times[1:])) if args.reps else times[0]
        if cuts is not None:
            res["cuts_device_equal_host"] = bool(np.array_equal(cuts[0], dcuts[0]) and np.array_equal(cuts[1], dcuts[1]))
        else:
            cuts = dcuts
    if args.cuts_full:
        fcuts, times = device_cuts(1)
        res["cuts_device_full_first_call_seconds"] = times[0]
        res["cuts_device_full_seconds"] = float(np.median(times[1:])) if args.reps else times[0]
        res["cuts_device_full_cut_values"] = int(fcuts[0][-1])
        res["cuts_full_plan"] = synth.cuts_plan(n, 1, F, cus)
    ncuts = int(cuts[0][-1])
    res["cut_values"] = ncuts
    if sampled and args.deep:
        n_sel = int(synth.boost_features(args.seed, 0, F, args.colsample).size)
        res["plan"] = synth.grow_plan_deep_sampled(n, F, n_sel, ncuts, args.max_depth, cus)
        res["sampling"] = {"subsample": args.subsample, "colsample_bytree": args.colsample, "seed": args.seed}
        res["deep"] = True
    elif sampled:
        res["plan"] = synth.grow_plan_sampled(n, F, args.colsample, ncuts, args.max_depth, cus)
        res["sampling"] = {"subsample": args.subsample, "colsample_bytree": args.colsample, "seed": args.seed}
    elif args.deep:
        res["plan"] = synth.grow_plan_deep(n, F, ncuts, args.max_depth, cus)
        res["deep"] = True
    else:
        res["plan"] = (synth.grow_plan if args.weights == "none" else synth.grow_plan_weighted)(n, F, ncuts, args.max_depth, cus)
    print("cuts", json.dumps({k: v for k, v in res.items() if k.startswith("cuts_") and not k.endswith("plan")}), flush=True)

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

    weights = None
    if args.weights == "ones":
        weights = torch.ones(n, dtype=torch.float32, device="cuda")
    elif args.weights == "random":
        weights = torch.rand(n, dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 4.0
    res["weights"] = args.weights
    res["objective"] = {"ohx_objective": args.objective, "ohx_huber_slope": args.huber_slope, "ohx_quantile_alpha": args.quantile_alpha,
                        "ohx_grow_pairs": args.pairs}
    res["regularisation"] = {"ohx_reg_alpha": args.reg_alpha, "ohx_max_delta_step": args.max_delta_step, "ohx_eval_metric": args.eval_metric}
    res["monotone_constraints"] = args.monotone
    res["interaction_constraints"] = args.interaction_constraints
    res["colsample"] = {"ohx_colsample_bylevel": args.colsample_bylevel, "ohx_colsample_bynode": args.colsample_bynode}
    res["pair_planes"] = synth.grow_pairs_plan(n, F, ncuts, args.max_depth, cus)

    def timed_booster():
        b = capi.Booster(model_buffer=model.image)
        b.set_param("ohx_objective", args.objective)
        b.set_param("ohx_huber_slope", repr(args.huber_slope))
        b.set_param("ohx_quantile_alpha", repr(args.quantile_alpha))
        b.set_param("ohx_grow_pairs", args.pairs)
        if regularised:        # (left unset otherwise: the tool then also runs against a library from before the parameters)
            b.set_param("ohx_reg_alpha", repr(args.reg_alpha))
            b.set_param("ohx_max_delta_step", repr(args.max_delta_step))
            b.set_param("ohx_eval_metric", args.eval_metric)
        if args.monotone is not None:
            b.set_param("ohx_monotone_constraints", args.monotone)
        if args.interaction_constraints is not None:
            b.set_param("ohx_interaction_constraints", args.interaction_constraints)
        if args.colsample_bylevel is not None:
            b.set_param("ohx_colsample_bylevel", repr(args.colsample_bylevel))
        if args.colsample_bynode is not None:
            b.set_param("ohx_colsample_bynode", repr(args.colsample_bynode))
        return b

    last = {}                              # what the weighted call returned last

    def boost(b, rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        if sampled:
            call = b.boost_trees_deep_sampled_device if args.deep else b.boost_trees_sampled_device
            r = call(d, labels.data_ptr(), n, cuts, weights_ptr=weights.data_ptr() if weights is not None else 0, rounds=rounds,
                     max_depth=args.max_depth, eta=args.eta, reg_lambda=args.reg_lambda, min_child_weight=1.0,
                     subsample=args.subsample, colsample_bytree=args.colsample, seed=args.seed, stream=stream)
            nodes = r["nodes_added"]
            last.update(rounds=rounds, train_rmse=r["train_rmse"].tolist())
        elif args.deep:
            r = b.boost_trees_deep_device(d, labels.data_ptr(), n, cuts, weights_ptr=weights.data_ptr() if weights is not None else 0,
                                          rounds=rounds, max_depth=args.max_depth, eta=args.eta, reg_lambda=args.reg_lambda,
                                          min_child_weight=1.0, stream=stream)
            nodes = r["nodes_added"]
            last.update(rounds=rounds, train_rmse=r["train_rmse"].tolist())
        elif weights is None:
            nodes = b.boost_trees_device(d, labels.data_ptr(), n, cuts, rounds=rounds, max_depth=args.max_depth, eta=args.eta,
                                         reg_lambda=args.reg_lambda, stream=stream)
        else:
            r = b.boost_trees_weighted_device(d, labels.data_ptr(), n, cuts, weights_ptr=weights.data_ptr(), rounds=rounds,
                                              max_depth=args.max_depth, eta=args.eta, reg_lambda=args.reg_lambda,
                                              min_child_weight=1.0, stream=stream)
            nodes = r["nodes_added"]
            last.update(rounds=rounds, train_rmse=r["train_rmse"].tolist())
        return time.perf_counter() - t, nodes

    if args.holdout:
        res["holdout"] = holdout(args, model, rows, labels, n, F, stream)
        print("holdout", json.dumps(res["holdout"]), flush=True)
    for rounds in ([] if args.holdout else sorted({1, args.rounds})):
        first, again, nodes = [], [], 0
        for _ in range(args.reps):
            b = timed_booster()
            dt, nodes = boost(b, rounds)
            first.append(dt)
            b.free()
            if args.deep_only:
                again.append(dt)
                continue
            # a call that finds its buffers: the second on one booster, continuing from the first
            b = timed_booster()
            boost(b, rounds)
            dt, _ = boost(b, rounds)
            again.append(dt)
            b.free()
        res[f"rounds_{rounds}"] = {"first_call_median_s": float(np.median(first)), "median_s": float(np.median(again)),
                                   "min_s": float(np.min(again)), "max_s": float(np.max(again)), "nodes_added": nodes}
        if last:
            res[f"rounds_{rounds}"]["train_rmse"] = last["train_rmse"]
        print(f"rounds_{rounds}", json.dumps(res[f"rounds_{rounds}"]), flush=True)
    if args.rounds > 1 and not args.holdout:
        per_round = (res[f"rounds_{args.rounds}"]["median_s"] - res["rounds_1"]["median_s"]) / (args.rounds - 1)
        res["per_round_s"] = per_round
        res["one_off_s"] = res["rounds_1"]["median_s"] - per_round
    if not args.skip_rmse and not args.holdout and not args.deep_only and args.objective == "squarederror" and not regularised and args.monotone is None and \
            args.interaction_constraints is None:
        b = capi.Booster(model_buffer=model.image)
        res["rmse_before"] = rmse(b)
        b.refit_leaves_device(d, labels.data_ptr(), n, eta=1.0, reg_lambda=1.0, stream=stream)
        res["rmse_after_refit"] = rmse(b)
        boost(b, args.rounds)
        res[f"rmse_after_refit_and_{args.rounds}_rounds"] = rmse(b)
        b.free()
    d.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
