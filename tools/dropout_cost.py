#!/usr/bin/env python3
"""Cost of dropout on the Products-shape step (2 x 8 heads x 8, fp32): per-kernel-class time from kernel_stats with dropout off,
attention dropout only, and attention + feature dropout, and the ratio of each to the default step.
    python tools/dropout_cost.py [--steps K] [--out FILE.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()

pkg = entry.load_package()
dev = torch.device("cuda", 0)
ds = pkg.synth.make_dataset_device("products", dev)
d_rp = torch.from_numpy(np.ascontiguousarray(ds["row_ptr"], np.int32)).to(dev)
settings = [("off", None), ("attention", (0.0, 0.5)), ("attention+features", (0.5, 0.5))]
res = {"workload": "products", "n": ds["n"], "e": ds["e"], "heads": [8, 8], "outdims": [8, 8], "steps": args.steps, "runs": {}}
with pkg.GatContext([8, 8], [8, 8], ds["f"], ds["c"], collect_timing=True) as ctx:
    ctx.set_graph_device(d_rp.data_ptr(), ds["d_col_idx"].data_ptr(), ds["n"], ds["e"])
    ctx.set_features_device(ds["d_x"].data_ptr(), ds["n"], ds["f"])
    ctx.set_labels_device(ds["d_labels"].data_ptr(), ds["n"])
    ctx.params_init(42)
    for name, p in settings:
        if p is None:
            ctx.set_dropout(0.0, 0.0, seed=1)
        else:
            ctx.set_dropout(p[0], p[1], seed=1)
        for _ in range(args.warmup):
            ctx.zero_grad(); ctx.step(want_loss=False)
        ctx.sync()
        ctx.kernel_stats_reset()
        for _ in range(args.steps):
            ctx.zero_grad(); ctx.step(want_loss=False)
        st = ctx.kernel_stats()
        per = {k: round(v[1] / args.steps, 4) for k, v in st.items() if v[0]}
        res["runs"][name] = {"ms_per_step": round(sum(per.values()), 4), "kernels_ms_per_step": per}
base = res["runs"]["off"]["ms_per_step"]
for name in res["runs"]:
    res["runs"][name]["ratio_to_off"] = round(res["runs"][name]["ms_per_step"] / base, 4)
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
