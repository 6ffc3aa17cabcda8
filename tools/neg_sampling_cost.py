#!/usr/bin/env python3
"""Cost of installing fresh negatives at the Products shape (2.45 M nodes, 61.9 M edges; `--pos` positives + `--neg` negative slots, 2 M
+ 2 M by default) — include/gatv2_abi.h "negative sampling".  One process, one pair context (mul, C = 1, BCE), `--warmup` untimed
rounds, then `--rounds` rounds that ALTERNATE the two ways, each call timed with the host clock around a call that ends in a synchronise:
  A  gat_set_pairs_device with a prepared device list of the same length — how new negatives are installed without the feature (the
     list itself would still have to be drawn and filtered on the host and uploaded: not counted);
  B  gat_resample_negatives(round): sampler + incidence sort + the device-built work list.
Reported: every round's time, median, min, max and spread (max - min) of both, and the decision figure B < A - spread(A).
The split of B into sampler / sort / plan is not visible to a host clock.  `--kernel-stats DIR` reads the *_kernel_stats.csv of a
SEPARATE run of this tool under `rocprofv3 --kernel-trace --stats` (its times are not used for A and B) and records the average
duration of the sampler kernel and of the plan's two kernels; the rest of B is the incidence sort with its allocations and host gaps.
Measured, never asserted.
    python tools/neg_sampling_cost.py [--workload products] [--scale S] [--pos A] [--neg B] [--mode uniform|corrupt] [--rounds R]
                                      [--warmup W] [--kernel-stats DIR] [--out profiles/neg_sampling/cost.json]"""
import argparse
import csv
import glob
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
ap.add_argument("--mode", default="uniform")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--kernel-stats", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

import torch  # noqa: E402

pkg = entry.load_package()
dev = torch.device("cuda:0")
heads, outdims = [8, 8], [8, 8]
dsd = pkg.synth.make_dataset_device(args.workload, dev, scale=args.scale)
n, e, f = dsd["n"], dsd["e"], dsd["f"]
d_rp = torch.from_numpy(dsd["row_ptr"]).to(dev)
u, v, t = pkg.synth.link_pairs(dsd["row_ptr"], dsd["d_col_idx"].cpu().numpy(), args.pos, args.neg, seed=42)
P = len(u)
d_u, d_v, d_t = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(t.reshape(P, 1)).to(dev)

ctx = pkg.GatContext(heads, outdims, f, 1)
ctx.set_loss("bce")
ctx.set_graph_device(d_rp.data_ptr(), dsd["d_col_idx"].data_ptr(), n, e)
ctx.set_features_device(dsd["d_x"].data_ptr(), n, f)
ctx.set_pairs_device("mul", d_u.data_ptr(), d_v.data_ptr(), P)
ctx.set_targets_device(d_t.data_ptr(), P, 1)
ctx.params_init(42)
ctx.zero_grad()
t0 = time.perf_counter()
ctx.set_negative_sampling(args.mode, args.pos, args.neg, seed=7)         # includes the one-pass "every row ascending" check
ctx.sync()
setup_ms = (time.perf_counter() - t0) * 1e3


def timed(fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return round((time.perf_counter() - t0) * 1e3, 3)


a_ms, b_ms, unfiltered = [], [], []
for r in range(args.warmup + args.rounds):
    ta = timed(lambda: ctx.set_pairs_device("mul", d_u.data_ptr(), d_v.data_ptr(), P))
    tb = timed(lambda: ctx.resample_negatives(r))
    ctx.step(want_loss=False)                            # the pair list is used between the rounds, as in training
    if r >= args.warmup:
        a_ms.append(ta); b_ms.append(tb); unfiltered.append(ctx.negatives_info()[4])
ctx.close()


def summary(x):
    return {"rounds_ms": x, "median_ms": round(statistics.median(x), 3), "min_ms": min(x), "max_ms": max(x), "spread_ms": round(max(x) - min(x), 3)}


res = {"workload": args.workload, "scale": args.scale, "n": n, "e": e, "n_pairs": P, "n_pos": args.pos, "n_neg": args.neg, "mode": args.mode,
       "rounds": args.rounds, "warmup": args.warmup, "set_negative_sampling_ms": round(setup_ms, 3),
       "A_set_pairs_device": summary(a_ms), "B_resample_negatives": summary(b_ms), "unfiltered_per_round": unfiltered}
A, B = res["A_set_pairs_device"], res["B_resample_negatives"]
res["decision"] = {"rule": "the device plan stays only if median B < median A - spread(A)",
                   "B_median_ms": B["median_ms"], "A_median_minus_spread_ms": round(A["median_ms"] - A["spread_ms"], 3),
                   "device_plan_stays": B["median_ms"] < A["median_ms"] - A["spread_ms"]}
if args.kernel_stats:
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*_kernel_stats.csv"), recursive=True)
    split = {}
    for row in csv.DictReader(open(files[0])) if files else []:
        for key in ("negative_sample_kernel", "pair_plan_keys_kernel", "pair_plan_fill_kernel", "pair_keys_kernel", "pair_entries_kernel"):
            if key in row["Name"]:
                split[key] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) * 1e-6, 5)}
    res["B_split_from_a_separate_trace_run"] = split or "not measured"
else:
    res["B_split_from_a_separate_trace_run"] = "not measured"
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
