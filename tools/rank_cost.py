#!/usr/bin/env python3
"""Cost of the ranking metrics at the Products shape (2.45 M nodes, 61.9 M edges) — include/gatv2_abi.h "ranking metrics".  Two heads:
  pair    the pair head of tools/pair_cost.py: `--pos` positives + `--neg` negatives (2 M + 2 M), C = 1, BCE
  node    the softmax node head, C = 47, every row in the mask
For each: one context, one forward, `--warmup` untimed rounds, then rounds that ALTERNATE the two ways, each timed with the host clock
around a call that ends in a synchronise:
  A  what a caller does without the feature: tap(GAT_TAP_Y) to the host plus tests/rank_ref.py (one numpy sort per column) — the thing to
     beat (`--host-rounds` of them: at C = 47 one takes many seconds);
  B  gat_eval_rank on the same context (`--rounds` of them).
and the bytes model of B: key build 4*slots read + 8*slots written; the radix sort at 16*slots per pass over ceil(bits / 8) passes,
compared with 6.3 TB/s; the prefix count 8*slots read + 4*slots written; the rank kernel's streamed reads 12*slots (its searches come on top).
The call's kernel classes come from SEPARATE runs of this tool, one per head, under `rocprofv3 --kernel-trace --output-format csv -d DIR`
(with --host-rounds 0; their times are not used for A and B): `--merge-trace pair=DIR,node=DIR --out FILE` then adds them to FILE without
touching a device.  Measured, never asserted.
    python tools/rank_cost.py [--heads pair,node] [--scale S] [--pos A] [--neg B] [--rounds R] [--host-rounds H] [--warmup W]
                              [--out profiles/rank_metrics/cost.json]
    python tools/rank_cost.py --merge-trace pair=DIR,node=DIR --out profiles/rank_metrics/cost.json"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--heads", default="pair,node")
ap.add_argument("--workload", default="products")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--pos", type=int, default=2000000)
ap.add_argument("--neg", type=int, default=2000000)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--host-rounds", type=int, default=2)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--merge-trace", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()


def trace_classes(directory):
    """The kernels of one gat_eval_rank from a rocprofv3 --kernel-trace run of this tool: every dispatch from a rank_keys_kernel to the next
    rank_finish_kernel is one call (the dataset's own sorts lie outside); averaged over the calls after the first."""
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if not files:
        return "not measured"
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "rank_keys_kernel" in name:
            cur = []
        if cur is not None:
            cur.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
            if "rank_finish_kernel" in name:
                calls.append(cur); cur = None
    calls = calls[1:] if len(calls) > 1 else calls
    if not calls:
        return "not measured"

    def cls(name):
        for key, c in (("rank_keys_kernel", "key build"), ("rank_columns_kernel", "columns + Hits@K"), ("rank_terms_kernel", "rank kernel"),
                       ("rank_finish_kernel", "finish"), ("scan", "prefix count")):
            if key in name.lower():
                return c
        return "radix sort"
    out = {}
    for call in calls:
        for name, ms in call:
            c = out.setdefault(cls(name), {"launches_per_call": 0.0, "ms_per_call": 0.0})
            c["launches_per_call"] += 1.0 / len(calls); c["ms_per_call"] += ms / len(calls)
    for c in out.values():
        c["launches_per_call"] = round(c["launches_per_call"], 2); c["ms_per_call"] = round(c["ms_per_call"], 4)
    return {"calls_averaged": len(calls), "classes": out, "kernel_ms_per_call": round(sum(c["ms_per_call"] for c in out.values()), 4)}


if args.merge_trace:                                 # no device: add the classes of earlier trace runs to an earlier result
    res = json.load(open(args.out))
    res["kernel_classes_from_a_separate_trace_run"] = {h: trace_classes(d) for h, d in (kv.split("=") for kv in args.merge_trace.split(","))}
    print(json.dumps(res["kernel_classes_from_a_separate_trace_run"]))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rank_ref as RR  # noqa: E402

pkg = entry.load_package()
A = pkg.abi
dev = torch.device("cuda:0")
KS = (10, 50, 100)
HBM_TBS = 6.3


def summary(x):
    if not x:
        return "not measured"
    return {"rounds_ms": x, "median_ms": round(statistics.median(x), 3), "min_ms": min(x), "max_ms": max(x), "spread_ms": round(max(x) - min(x), 3)}


def bytes_model(slots, C):
    bits = 33 + max(1, int(C).bit_length())
    passes = math.ceil(bits / 8)
    parts = {"key_build": 12 * slots, "sort": 16 * slots * passes, "prefix_count": 12 * slots, "rank_kernel_streamed": 12 * slots}
    total = sum(parts.values())
    return {"slots": slots, "key_bits": bits, "sort_passes_of_8_bits": passes, "bytes": parts, "bytes_total": total,
            "ms_at_%.1f_TBs" % HBM_TBS: round(total / (HBM_TBS * 1e12) * 1e3, 4),
            "sort_ms_at_%.1f_TBs" % HBM_TBS: round(parts["sort"] / (HBM_TBS * 1e12) * 1e3, 4)}


def measure(ctx, rows, C, labels, targets):
    mask = np.ones(rows, np.uint8)

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return round((time.perf_counter() - t0) * 1e3, 3), out

    def host():
        y = ctx.tap(A.TAP_Y).reshape(rows, C)
        return RR.rank_stats(y, labels=labels, targets=targets, mask=mask, ks=KS)

    ctx.forward(want_loss=False)
    a_ms, b_ms, got, want = [], [], None, None
    for r in range(args.warmup + max(args.rounds, args.host_rounds)):
        if r - args.warmup < args.rounds:
            tb, got = timed(lambda: ctx.eval_rank(mask, KS))
            if r >= args.warmup:
                b_ms.append(tb)
        if r >= args.warmup and r - args.warmup < args.host_rounds:
            ta, want = timed(host)
            a_ms.append(ta)
    agree = "not compared"
    if want is not None and got is not None:
        RR.assert_same(got, want, "rank_cost")
        agree = True
    both = (got["n_pos"] > 0) & (got["n_neg"] > 0)
    return {"rows": rows, "C": C, "A_tap_plus_numpy": summary(a_ms), "B_gat_eval_rank": summary(b_ms), "device_equals_reference": agree,
            "columns_with_both_classes": int(both.sum()), "macro_auc": float(np.mean(got["auc"][both])) if both.any() else None,
            "bytes_model": bytes_model(rows * C, C)}


res = {"workload": args.workload, "scale": args.scale, "rounds": args.rounds, "host_rounds": args.host_rounds, "warmup": args.warmup, "ks": list(KS)}
dsd = pkg.synth.make_dataset_device(args.workload, dev, scale=args.scale)
n, e, f = dsd["n"], dsd["e"], dsd["f"]
res.update(n=n, e=e)
d_rp = torch.from_numpy(dsd["row_ptr"]).to(dev)
for head in args.heads.split(","):
    if head == "pair":
        u, v, t = pkg.synth.link_pairs(dsd["row_ptr"], dsd["d_col_idx"].cpu().numpy(), args.pos, args.neg, seed=42)
        P = len(u)
        d_u, d_v, d_t = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(t.reshape(P, 1)).to(dev)
        ctx = pkg.GatContext([8, 8], [8, 8], f, 1)
        ctx.set_loss("bce")
        ctx.set_graph_device(d_rp.data_ptr(), dsd["d_col_idx"].data_ptr(), n, e)
        ctx.set_features_device(dsd["d_x"].data_ptr(), n, f)
        ctx.set_pairs_device("mul", d_u.data_ptr(), d_v.data_ptr(), P)
        ctx.set_targets_device(d_t.data_ptr(), P, 1)
        ctx.params_init(42)
        res["pair"] = measure(ctx, P, 1, None, np.asarray(t, np.float32).reshape(P, 1))
        ctx.close()
    elif head == "node":
        C = dsd["c"]
        labels = dsd["d_labels"].cpu().numpy()
        ctx = pkg.GatContext([8, 8], [8, 8], f, C)
        ctx.set_graph_device(d_rp.data_ptr(), dsd["d_col_idx"].data_ptr(), n, e)
        ctx.set_features_device(dsd["d_x"].data_ptr(), n, f)
        ctx.set_labels_device(dsd["d_labels"].data_ptr(), n)
        ctx.params_init(42)
        res["node"] = measure(ctx, n, C, labels, None)
        ctx.close()

res["kernel_classes_from_a_separate_trace_run"] = "not measured"
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
