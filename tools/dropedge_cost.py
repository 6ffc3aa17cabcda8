#!/usr/bin/env python3
"""Cost of DropEdge on the Products-shape step (2 x 8 heads x 8, fp32): forward + backward time per step with DropEdge off, at
p_e = 0.1 and 0.5, at p_e = 0.5 together with attention dropout 0.5, and with attention dropout 0.5 alone.  All settings run in
ONE process on ONE context, interleaved A/B/A...: `--rounds` passes over the list of settings, each pass timing `--steps` steps of
every setting after `--warmup` untimed ones (a change of setting re-arms the kernels' code and the caches), wall time between two
stream synchronisations.  Per setting the file holds every round's ms/step, their median and min / max; the spread of "off" over
the rounds is the noise the other numbers are to be read against.
    python tools/dropedge_cost.py [--steps K] [--warmup W] [--rounds R] [--out profiles/dropedge/cost.json]"""
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
ap.add_argument("--out", default="")
args = ap.parse_args()

pkg = entry.load_package()
dev = torch.device("cuda", 0)
ds = pkg.synth.make_dataset_device("products", dev)
d_rp = torch.from_numpy(np.ascontiguousarray(ds["row_ptr"], np.int32)).to(dev)
# (name, p_edge, p_attn)
settings = [("off", 0.0, 0.0), ("dropedge_0.1", 0.1, 0.0), ("dropedge_0.5", 0.5, 0.0), ("dropedge_0.5+attention_0.5", 0.5, 0.5),
            ("attention_0.5", 0.0, 0.5)]
res = {"workload": "products", "n": ds["n"], "e": ds["e"], "heads": [8, 8], "outdims": [8, 8], "steps": args.steps,
       "warmup": args.warmup, "rounds": args.rounds, "gather_skip_variant": "not built (see profiles/dropedge/resource_usage.md)",
       "runs": {name: {"ms_per_step_rounds": []} for name, _, _ in settings}}
with pkg.GatContext([8, 8], [8, 8], ds["f"], ds["c"]) as ctx:
    ctx.set_graph_device(d_rp.data_ptr(), ds["d_col_idx"].data_ptr(), ds["n"], ds["e"])
    ctx.set_features_device(ds["d_x"].data_ptr(), ds["n"], ds["f"])
    ctx.set_labels_device(ds["d_labels"].data_ptr(), ds["n"])
    ctx.params_init(42)
    for _ in range(args.rounds):
        for name, pe, pa in settings:
            ctx.set_dropout(0.0, pa, seed=1)
            ctx.set_dropedge(pe)
            for _ in range(args.warmup):
                ctx.zero_grad(); ctx.step(want_loss=False)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.zero_grad(); ctx.step(want_loss=False)
            ctx.sync()
            res["runs"][name]["ms_per_step_rounds"].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 4))
for name in res["runs"]:
    r = res["runs"][name]["ms_per_step_rounds"]
    res["runs"][name].update(ms_per_step=round(statistics.median(r), 4), min=min(r), max=max(r))
base = res["runs"]["off"]["ms_per_step"]
for name in res["runs"]:
    res["runs"][name]["ratio_to_off"] = round(res["runs"][name]["ms_per_step"] / base, 4)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
