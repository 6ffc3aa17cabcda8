#!/usr/bin/env python3
"""Cost of batch normalisation on the Products-shape step (2 x 8 heads x 8, fp32): forward + backward time per step with the feature
off, with layer normalisation on the hidden layer, and with batch normalisation on the hidden layer (GAT_BN_SKIP_LAST — where DGL's OGB
baselines put it).  Every setting has a context of its own (the setters fix the packed buffers before the graph is set); all live in
ONE process and run interleaved A/B/C/A...: `--rounds` passes over the settings, each timing `--steps` steps of every setting after
`--warmup` untimed ones, wall time between two stream synchronisations.  Per setting the file holds every round's ms/step, their median
and min / max, the ratio to "off" of the same process, the context's algorithmic bytes and — from the contexts' own event timing, in a
pass of its own after the wall-clock rounds — the GAT_K_MISC class per step (launches and ms).  The split of that class by kernel comes
from a kernel trace of `--only batch_norm` (profiles/batch_norm/README.md says how it was taken).
    python tools/batchnorm_cost.py [--steps K] [--warmup W] [--rounds R] [--only NAME] [--out profiles/batch_norm/cost.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--only", default="", help="run this setting alone (for a kernel trace)")
ap.add_argument("--out", default="")
args = ap.parse_args()

pkg = entry.load_package()
A = pkg.abi
dev = torch.device("cuda", 0)
ds = pkg.synth.make_dataset_device("products", dev)
d_rp = torch.from_numpy(np.ascontiguousarray(ds["row_ptr"], np.int32)).to(dev)
settings = [s for s in ("off", "layer_norm", "batch_norm") if not args.only or s == args.only]
res = {"workload": "products", "n": ds["n"], "e": ds["e"], "heads": [8, 8], "outdims": [8, 8], "steps": args.steps,
       "warmup": args.warmup, "rounds": args.rounds, "normalised_layers": "hidden layer only (skip_last)",
       "runs": {name: {"ms_per_step_rounds": []} for name in settings}}


def make(name, timing):
    ctx = pkg.GatContext([8, 8], [8, 8], ds["f"], ds["c"], collect_timing=timing)
    if name == "layer_norm":
        ctx.set_norm(skip_last=True)
    elif name == "batch_norm":
        ctx.set_batch_norm(skip_last=True)
    ctx.set_graph_device(d_rp.data_ptr(), ds["d_col_idx"].data_ptr(), ds["n"], ds["e"])
    ctx.set_features_device(ds["d_x"].data_ptr(), ds["n"], ds["f"])
    ctx.set_labels_device(ds["d_labels"].data_ptr(), ds["n"])
    ctx.params_init(42)
    return ctx


ctxs = {}
try:
    for name in settings:
        ctxs[name] = make(name, False)
        res["runs"][name]["algorithmic_bytes"] = ctxs[name].algorithmic_bytes()[0]
    for _ in range(args.rounds):
        for name in settings:
            ctx = ctxs[name]
            for _ in range(args.warmup):
                ctx.zero_grad(); ctx.step(want_loss=False)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.zero_grad(); ctx.step(want_loss=False)
            ctx.sync()
            res["runs"][name]["ms_per_step_rounds"].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 4))
finally:
    for ctx in ctxs.values():
        ctx.close()
for name in settings:                                # the misc class per step, from event pairs (they serialise the launches: not in the rounds above)
    with make(name, True) as ctx:
        for _ in range(args.warmup):
            ctx.zero_grad(); ctx.step(want_loss=False)
        ctx.sync()
        ctx.kernel_stats_reset()
        for _ in range(args.steps):
            ctx.zero_grad(); ctx.step(want_loss=False)
        ctx.sync()
        stats = ctx.kernel_stats()
        launches, ms = stats[A.load_library().gat_kernel_name(A.K_MISC).decode()]
        res["runs"][name]["misc_launches_per_step"] = launches / args.steps
        res["runs"][name]["misc_ms_per_step"] = round(ms / args.steps, 4)
for name in settings:
    r = res["runs"][name]["ms_per_step_rounds"]
    res["runs"][name].update(ms_per_step=round(statistics.median(r), 4), min=min(r), max=max(r))
if "off" in res["runs"]:
    base = res["runs"]["off"]
    for name in settings:
        res["runs"][name]["ratio_to_off"] = round(res["runs"][name]["ms_per_step"] / base["ms_per_step"], 4)
        res["runs"][name]["ms_over_off"] = round(res["runs"][name]["ms_per_step"] - base["ms_per_step"], 4)
        res["runs"][name]["bytes_over_off"] = res["runs"][name]["algorithmic_bytes"] - base["algorithmic_bytes"]
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
