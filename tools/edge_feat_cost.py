#!/usr/bin/env python3
"""Cost of edge features on the Products-shape step (2 x 8 heads x 8, fp32): forward + backward time per step with the feature off
and with edge_dim = Fe (default 8; attribute rows of synth.edge_features).  gat_set_edge_dim fixes the packed parameter buffers before
the graph is set, so each setting has a context of its own; both live in ONE process and run interleaved A/B/A/B...: `--rounds`
passes over the settings, each pass timing `--steps` steps of every setting after `--warmup` untimed ones, wall time between two
stream synchronisations.  Per setting the file holds every round's ms/step, their median and min / max, the ratio to "off" of the
same process, and the context's algorithmic bytes with their increase over "off" (include/gatv2_abi.h "edge features" says which
terms the feature adds: a dense per-edge row read by both edge passes and written by the backward); the spread of "off" over the
rounds is the noise the other numbers are to be read against.  The "on" context holds (L + 1) * E * H*D * 4 bytes more than "off"
(47.5 GB at this shape) plus the attribute rows.
    python tools/edge_feat_cost.py [--fe Fe] [--steps K] [--warmup W] [--rounds R] [--out profiles/edge_features/cost.json]"""
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
ap.add_argument("--fe", type=int, default=8)
ap.add_argument("--out", default="")
args = ap.parse_args()

pkg = entry.load_package()
dev = torch.device("cuda", 0)
ds = pkg.synth.make_dataset_device("products", dev)
d_rp = torch.from_numpy(np.ascontiguousarray(ds["row_ptr"], np.int32)).to(dev)
# (name, edge_dim)
settings = [("off", 0), (f"fe{args.fe}", args.fe)]
res = {"workload": "products", "n": ds["n"], "e": ds["e"], "heads": [8, 8], "outdims": [8, 8], "edge_dim": args.fe, "steps": args.steps,
       "warmup": args.warmup, "rounds": args.rounds, "runs": {name: {"ms_per_step_rounds": []} for name, _ in settings}}
ctxs = {}
try:
    for name, fe in settings:
        ctx = pkg.GatContext([8, 8], [8, 8], ds["f"], ds["c"])
        ctxs[name] = ctx
        ctx.set_edge_dim(fe)
        ctx.set_graph_device(d_rp.data_ptr(), ds["d_col_idx"].data_ptr(), ds["n"], ds["e"])
        ctx.set_features_device(ds["d_x"].data_ptr(), ds["n"], ds["f"])
        ctx.set_labels_device(ds["d_labels"].data_ptr(), ds["n"])
        if fe:
            ctx.set_edge_features(pkg.synth.edge_features(42, ds["e"], fe))
        ctx.params_init(42)
        res["runs"][name]["algorithmic_bytes"] = ctx.algorithmic_bytes()[0]
    for _ in range(args.rounds):
        for name, _ in settings:
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
for name in res["runs"]:
    r = res["runs"][name]["ms_per_step_rounds"]
    res["runs"][name].update(ms_per_step=round(statistics.median(r), 4), min=min(r), max=max(r))
base = res["runs"]["off"]["ms_per_step"]
for name in res["runs"]:
    res["runs"][name]["ratio_to_off"] = round(res["runs"][name]["ms_per_step"] / base, 4)
    res["runs"][name]["bytes_ratio_to_off"] = round(res["runs"][name]["algorithmic_bytes"] / res["runs"]["off"]["algorithmic_bytes"], 4)
    res["runs"][name]["bytes_over_off"] = res["runs"][name]["algorithmic_bytes"] - res["runs"]["off"]["algorithmic_bytes"]
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
