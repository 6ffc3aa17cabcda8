#!/usr/bin/env python3
"""Cost of the BCE / MSE output heads at the Products shape (2.45 M nodes, 61.9 M edges, C = 47, 2 layers x 8 heads x 8, fp32) against
the softmax head IN THE SAME RUN (include/gatv2_abi.h "loss modes of the output head").  gat_set_loss fixes the head's buffers and
kernels, so each setting has a context of its own; the three live in ONE process and run interleaved: `--rounds` passes over the
settings, each pass running `--steps` steps of every setting after `--warmup` untimed ones.  Two passes of their own:
  1. wall clock per step (sync, steps, sync) with collect_timing off — what a training loop sees;
  2. collect_timing on: the head classes' own time per step (HIP-event pairs around every launch, gat_kernel_stats):
     head_forward + head_backward.
The yardstick is the softmax head's class time of this run: the new heads do less arithmetic per entry and stream 4 * N * C more bytes
of targets per reading pass, so their class time should not exceed softmax's + those bytes / 6.3 TB/s + max(10 %, the spread of the
softmax rounds).  The file holds every round, the medians, the allowance and whether each mode is inside it.  Measured, never asserted.
GAT_LOSS_BLOCKED=0 in the environment measures the any-shape form of the new kernels where the register-blocked form is the default.
    python tools/loss_cost.py [--workload products] [--scale S] [--steps K] [--warmup W] [--rounds R] [--out profiles/loss_modes/cost.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="products")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--missing", type=float, default=0.2)
ap.add_argument("--out", default="")
args = ap.parse_args()

import torch  # noqa: E402

pkg = entry.load_package()
dev = torch.device("cuda:0")
heads, outdims = [8, 8], [8, 8]
dsd = pkg.synth.make_dataset_device(args.workload, dev, scale=args.scale)
n, e, f, c = dsd["n"], dsd["e"], dsd["f"], dsd["c"]
d_rp = torch.from_numpy(dsd["row_ptr"]).to(dev)
gen = torch.Generator(device=dev)
gen.manual_seed(42)
hole = torch.rand((n, c), device=dev, generator=gen) < args.missing
d_t = {"bce": (torch.rand((n, c), device=dev, generator=gen) < 0.5).float(), "mse": torch.rand((n, c), device=dev, generator=gen) * 2 - 1}
for t in d_t.values():
    t[hole] = float("nan")
del hole
settings = ["softmax", "bce", "mse"]
HBM = 6.3e12          # practical streaming ceiling (README)
res = {"workload": args.workload, "scale": args.scale, "n": n, "e": e, "f": f, "c": c, "heads": heads, "outdims": outdims, "missing": args.missing,
       "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "switches": "",
       "runs": {name: {"wall_ms_per_step_rounds": [], "head_ms_rounds": [], "class_ms_rounds": []} for name in settings}}


def build(name, timing):
    ctx = pkg.GatContext(heads, outdims, f, c, collect_timing=timing)
    ctx.set_loss(name)
    ctx.set_graph_device(d_rp.data_ptr(), dsd["d_col_idx"].data_ptr(), n, e)
    ctx.set_features_device(dsd["d_x"].data_ptr(), n, f)
    if name == "softmax":
        ctx.set_labels_device(dsd["d_labels"].data_ptr(), n)
    else:
        ctx.set_targets_device(d_t[name].data_ptr(), n, c)
    ctx.params_init(42)
    ctx.zero_grad()
    return ctx


for timing in (False, True):
    ctxs = {}
    try:
        for name in settings:
            ctxs[name] = build(name, timing)
            if timing:
                tot, per = ctxs[name].algorithmic_bytes()
                res["runs"][name]["algorithmic_bytes"] = tot
                res["runs"][name]["algorithmic_bytes_head"] = per["head_forward"] + per["head_backward"]
        for _ in range(args.rounds):
            for name in settings:
                ctx = ctxs[name]
                for _ in range(args.warmup):
                    ctx.zero_grad(); ctx.step(want_loss=False)
                ctx.sync()
                ctx.kernel_stats_reset()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    ctx.zero_grad(); ctx.step(want_loss=False)
                ctx.sync()
                dt = time.perf_counter() - t0
                run = res["runs"][name]
                if not timing:
                    run["wall_ms_per_step_rounds"].append(round(1e3 * dt / args.steps, 4))
                else:
                    per = {k: round(v[1] / args.steps, 5) for k, v in ctx.kernel_stats().items() if v[0]}
                    run["class_ms_rounds"].append(per)
                    run["head_ms_rounds"].append(round(per.get("head_forward", 0.0) + per.get("head_backward", 0.0), 5))
    finally:
        for ctx in ctxs.values():
            ctx.close()
for name in settings:
    run = res["runs"][name]
    run["wall_ms_per_step"] = round(statistics.median(run["wall_ms_per_step_rounds"]), 4)
    run["head_ms"] = round(statistics.median(run["head_ms_rounds"]), 5)
soft = res["runs"]["softmax"]
spread = (max(soft["head_ms_rounds"]) - min(soft["head_ms_rounds"])) / soft["head_ms"] if soft["head_ms"] else 0.0
# a step without keep_taps reads the targets once (the fused gradient kernel): 4 * N * C bytes more than the labels' 4 * N
extra_ms = 1e3 * 4.0 * n * (c - 1) / HBM
res["yardstick"] = {"softmax_head_ms": soft["head_ms"], "softmax_spread": round(spread, 4), "target_bytes_ms": round(extra_ms, 5),
                    "margin": round(max(0.10, spread), 4)}
for name in ("bce", "mse"):
    allow = soft["head_ms"] * (1.0 + max(0.10, spread)) + extra_ms
    res["runs"][name]["allowance_ms"] = round(allow, 5)
    res["runs"][name]["inside_allowance"] = res["runs"][name]["head_ms"] <= allow
    res["runs"][name]["wall_ratio_to_softmax"] = round(res["runs"][name]["wall_ms_per_step"] / soft["wall_ms_per_step"], 4)
res["switches"] = pkg.abi.switches()         # e.g. GAT_LOSS_BLOCKED=0: the any-shape form of the new head kernels at every shape (A/B)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
