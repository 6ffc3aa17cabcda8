#!/usr/bin/env python3
"""Cost of the hidden layer in front of the output head at the Products shape (2.45 M nodes, 61.9 M edges, 2 layers x 8 heads x 8, fp32,
D_last = 8): a link-prediction step — pair head MUL, synth.link_pairs with `--pos` positives + `--neg` negatives (2 M + 2 M by default),
C = 1, BCE — without the hidden stage and with Dh = 64 and Dh = 256 IN THE SAME RUN (include/gatv2_abi.h "hidden layer").
gat_set_head_hidden sizes the packed buffers, so each setting has a context of its own; the three live in ONE process and run
interleaved: `--rounds` passes over the settings, each pass running `--steps` steps of every setting after `--warmup` untimed ones.
Two passes of their own:
  1. wall clock per step (sync, steps, sync) with collect_timing off — what a training loop sees;
  2. collect_timing on: the head classes' own time per step (HIP-event pairs around every launch, gat_kernel_stats).  The stage's
     forward launches (the product A, the activation kernel) are timed under head_forward with the gather; its backward launches (the
     activation backward, gradb1's reduction, gradW1, the memset and gXin) under head_backward with the head's fused kernel and the scatter.
The two new row-streaming kernels' own times are not separable from their classes through gat_kernel_stats: they come from a
kernel trace of `--trace-pass` (this script run once more under the profiler with that flag: only the two hidden settings, a few
steps, no timing), whose per-dispatch trace `--kernel-stats FILE` merges into the result: each kernel's median time per width against its
bytes (2 R Dh 4 forward, 3 R Dh 4 backward) at the 6.3 TB/s practical ceiling.  Measured, never asserted.
    python tools/head_mlp_cost.py [--workload products] [--scale S] [--pos A] [--neg B] [--steps K] [--warmup W] [--rounds R]
                                  [--trace-pass] [--kernel-stats FILE] [--out profiles/head_mlp/cost.json]"""
import argparse
import csv
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
ap.add_argument("--pos", type=int, default=2000000)
ap.add_argument("--neg", type=int, default=2000000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--trace-pass", action="store_true")
ap.add_argument("--kernel-stats", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

HBM = 6.3e12          # practical streaming ceiling (README)
WIDTHS = {"none": 0, "dh64": 64, "dh256": 256}


def merge_kernel_stats(res, path):
    """The kernel trace of a --trace-pass run (CSV, one row per dispatch: Kernel_Name, Start_Timestamp, End_Timestamp in ns) -> each new
    kernel's time per width against its bytes.  The trace pass runs the Dh = 64 context's steps first and the Dh = 256 context's after
    them, the same number of each: the first half of a kernel's dispatches (by start time) is the first width's."""
    rows = list(csv.DictReader(open(path)))
    P = res["n_pairs"]
    widths = res.get("trace_widths", [64, 256])
    out = {}
    for key, mult in (("head_hidden_forward_kernel", 2), ("head_hidden_backward_kernel", 3)):
        hit = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if key in r.get("Kernel_Name", "")))
        if not hit or len(hit) % len(widths):
            continue
        per = len(hit) // len(widths)
        for i, Dh in enumerate(widths):
            d = [e - s for s, e in hit[i * per:(i + 1) * per]]
            med_s = statistics.median(d) * 1e-9
            nbytes = mult * P * Dh * 4.0
            out[f"{key} Dh={Dh}"] = {"calls": per, "median_us": round(med_s * 1e6, 3), "min_us": round(min(d) * 1e-3, 3), "bytes": nbytes,
                                     "achieved_TBps": round(nbytes / med_s / 1e12, 4), "fraction_of_6.3TBps": round(nbytes / med_s / HBM, 4)}
    res["kernels"] = out


if args.kernel_stats and args.out and os.path.exists(args.out) and not args.trace_pass:
    # merge mode: the timing run wrote args.out earlier; add the trace's figures
    res = json.load(open(args.out))
    merge_kernel_stats(res, args.kernel_stats)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res.get("kernels", {})))
    sys.exit(0)

import torch  # noqa: E402

pkg = entry.load_package()
dev = torch.device("cuda:0")
heads, outdims = [8, 8], [8, 8]
DL = outdims[-1]
dsd = pkg.synth.make_dataset_device(args.workload, dev, scale=args.scale)
n, e, f = dsd["n"], dsd["e"], dsd["f"]
d_rp = torch.from_numpy(dsd["row_ptr"]).to(dev)
u, v, t = pkg.synth.link_pairs(dsd["row_ptr"], dsd["d_col_idx"].cpu().numpy(), args.pos, args.neg, seed=42)
P = len(u)
d_u, d_v, d_t = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(t.reshape(P, 1)).to(dev)
settings = ["dh64", "dh256"] if args.trace_pass else list(WIDTHS)
res = {"workload": args.workload, "scale": args.scale, "n": n, "e": e, "f": f, "c": 1, "loss": "bce", "pairs": "mul", "heads": heads,
       "outdims": outdims, "n_pairs": P, "n_pos": args.pos, "n_neg": args.neg, "steps": args.steps, "warmup": args.warmup,
       "rounds": args.rounds, "trace_widths": [64, 256],
       "runs": {name: {"width": WIDTHS[name], "wall_ms_per_step_rounds": [], "class_ms_rounds": []} for name in settings}}


def build(name, timing):
    ctx = pkg.GatContext(heads, outdims, f, 1, collect_timing=timing)
    ctx.set_loss("bce")
    if WIDTHS[name]:
        ctx.set_head_hidden(WIDTHS[name])
    ctx.set_graph_device(d_rp.data_ptr(), dsd["d_col_idx"].data_ptr(), n, e)
    ctx.set_features_device(dsd["d_x"].data_ptr(), n, f)
    ctx.set_pairs_device("mul", d_u.data_ptr(), d_v.data_ptr(), P)
    ctx.set_targets_device(d_t.data_ptr(), P, 1)
    ctx.params_init(42)
    ctx.zero_grad()
    return ctx


if args.trace_pass:                                      # under the profiler: the launches only
    for name in settings:
        ctx = build(name, False)
        for _ in range(args.warmup + args.steps):
            ctx.zero_grad(); ctx.step(want_loss=False)
        ctx.sync()
        ctx.close()
    print(json.dumps({"trace_pass": settings, "steps": args.warmup + args.steps}))
    sys.exit(0)

for timing in (False, True):
    ctxs = {}
    try:
        for name in settings:
            ctxs[name] = build(name, timing)
            if timing:
                tot, per = ctxs[name].algorithmic_bytes()
                res["runs"][name]["algorithmic_bytes"] = tot
                res["runs"][name]["algorithmic_bytes_classes"] = per
        for _ in range(args.rounds):
            for name in settings:
                ctx = ctxs[name]
                for _ in range(args.warmup):
                    ctx.zero_grad(); ctx.step(want_loss=False)
                ctx.sync()
                if timing:
                    ctx.kernel_stats_reset()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    ctx.zero_grad(); ctx.step(want_loss=False)
                ctx.sync()
                wall = (time.perf_counter() - t0) * 1e3 / args.steps
                if timing:
                    res["runs"][name]["class_ms_rounds"].append({k: round(s[1] / args.steps, 5) for k, s in ctx.kernel_stats().items() if s[0]})
                else:
                    res["runs"][name]["wall_ms_per_step_rounds"].append(round(wall, 4))
    finally:
        for ctx in ctxs.values():
            ctx.close()

for name in settings:
    run = res["runs"][name]
    run["wall_ms_per_step"] = round(statistics.median(run["wall_ms_per_step_rounds"]), 4)
    run["class_ms"] = {k: round(statistics.median(c[k] for c in run["class_ms_rounds"]), 5) for k in run["class_ms_rounds"][0]}
base = res["runs"]["none"]
for name in settings:
    run = res["runs"][name]
    run["wall_ratio_to_none"] = round(run["wall_ms_per_step"] / base["wall_ms_per_step"], 4)
    Dh = run["width"]
    if Dh:
        run["stage_bytes"] = {"head_forward": 4.0 * (P * DL + Dh * DL + 3 * P * Dh),
                              "head_backward": 4.0 * (3 * P * Dh + (P * Dh + P * DL + Dh * DL) + (P * Dh + Dh * DL + P * DL))}
        run["class_ms_over_none"] = {k: round(run["class_ms"].get(k, 0.0) - base["class_ms"].get(k, 0.0), 5) for k in ("head_forward", "head_backward")}
if args.kernel_stats:
    merge_kernel_stats(res, args.kernel_stats)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
