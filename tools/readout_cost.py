#!/usr/bin/env python3
"""Cost of the graph-level readout on a molecule-like batch (synth.graph_batch: by default 100 k graphs of 10-40 nodes, average
in-degree 4; 2 layers x 8 heads x 8, fp32): forward + backward of one step with readout off (one label per node), mean and max.
gat_set_readout sizes the label and head buffers, so each setting has a context of its own; all three live in ONE process and run
interleaved: `--rounds` passes over the settings, each pass running `--steps` steps of every setting after `--warmup` untimed ones.
Times are the context's own kernel classes (collect_timing: HIP-event pairs around every launch, gat_kernel_stats), per step: the pool
kernel is timed under head_forward, the un-pool under head_backward.  Per setting the file holds every round's summed ms/step, its
median, min / max, the per-class medians, and the context's algorithmic bytes (include/gatv2_abi.h "graph-level readout": the head
priced with G rows, misc + 2 * 4 * (N + G) * D_last); the spread of "off" over the rounds is the noise the rest is to be read against.
Measured once, never asserted.
    python tools/readout_cost.py [--graphs G] [--lo A] [--hi B] [--degree D] [--steps K] [--warmup W] [--rounds R] [--out profiles/readout/cost.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--graphs", type=int, default=100000)
ap.add_argument("--lo", type=int, default=10)
ap.add_argument("--hi", type=int, default=40)
ap.add_argument("--degree", type=float, default=4.0)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()

pkg = entry.load_package()
heads, outdims = [8, 8], [8, 8]
ds = pkg.synth.graph_batch(args.graphs, args.lo, args.hi, args.degree, seed=42)
node_labels = pkg.synth.labels(ds["n"], ds["c"])
settings = ["off", "mean", "max"]
res = {"workload": "graph_batch", "n_graphs": ds["n_graphs"], "nodes": [args.lo, args.hi], "avg_degree": args.degree, "n": ds["n"], "e": ds["e"],
       "f": ds["f"], "c": ds["c"], "heads": heads, "outdims": outdims, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
       "runs": {name: {"ms_per_step_rounds": [], "class_ms_rounds": []} for name in settings}}
ctxs = {}
try:
    for name in settings:
        ctx = pkg.GatContext(heads, outdims, ds["f"], ds["c"], collect_timing=True)
        ctxs[name] = ctx
        ctx.set_graph(ds["row_ptr"], ds["col_idx"])
        ctx.set_features(ds["x"])
        if name != "off":
            ctx.set_readout(name, graph_ptr=ds["graph_ptr"])
        ctx.set_labels(node_labels if name == "off" else ds["labels"])
        ctx.params_init(42)
        tot, per = ctx.algorithmic_bytes()
        res["runs"][name]["algorithmic_bytes"] = tot
        res["runs"][name]["algorithmic_bytes_classes"] = per
    for _ in range(args.rounds):
        for name in settings:
            ctx = ctxs[name]
            for _ in range(args.warmup):
                ctx.zero_grad(); ctx.step(want_loss=False)
            ctx.sync()
            ctx.kernel_stats_reset()
            for _ in range(args.steps):
                ctx.zero_grad(); ctx.step(want_loss=False)
            ctx.sync()
            per = {k: round(v[1] / args.steps, 5) for k, v in ctx.kernel_stats().items() if v[0]}
            res["runs"][name]["class_ms_rounds"].append(per)
            res["runs"][name]["ms_per_step_rounds"].append(round(sum(per.values()), 4))
finally:
    for ctx in ctxs.values():
        ctx.close()
for name in settings:
    run = res["runs"][name]
    r = run["ms_per_step_rounds"]
    run.update(ms_per_step=round(statistics.median(r), 4), min=min(r), max=max(r))
    run["class_ms"] = {k: round(statistics.median(c[k] for c in run["class_ms_rounds"]), 5) for k in run["class_ms_rounds"][0]}
off = res["runs"]["off"]
for name in settings:
    run = res["runs"][name]
    run["ratio_to_off"] = round(run["ms_per_step"] / off["ms_per_step"], 4)
    run["bytes_over_off"] = run["algorithmic_bytes"] - off["algorithmic_bytes"]
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
