#!/usr/bin/env python3
"""Wall clock per epoch of the three ways to run a training epoch with Adam and per-group clipping, on the Cora-, Pubmed- and Arxiv-shape
synthetic configs of BASELINE (2 / 2 / 3 layers of 8 heads x 8, fp32), all with the step as a replayed graph (step_graph):
    a  zero_grad, step (replay), clip, step_adam         the sequence train_edge makes without the new flags: up to 2 launches per
                                                         live group for the clip, one for Adam, one memset — behind the one-launch replay
    b  zero_grad, step (replay), optimizer_step          clip and update in two launches
    c  train_step (replay)                               zero, step, clip and update in the ONE replayed launch
Every variant has a context of its own; all nine live in ONE process and run interleaved (a/b/c per workload, workload by workload):
`--rounds` passes, each timing `--steps` epochs of every variant after `--warmup` untimed ones, wall time between two stream
synchronisations.  Per variant the file holds every round's ms/epoch, their median and min / max and the ratio to (a) of the same
process.  (a) is the yardstick: the code path of the parent commit, present unchanged.
    python tools/optimizer_cost.py [--steps K] [--warmup W] [--rounds R] [--workloads cora,pubmed,arxiv] [--out profiles/optimizer/cost.json]"""
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
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--workloads", default="cora,pubmed,arxiv")
ap.add_argument("--out", default="")
args = ap.parse_args()

pkg = entry.load_package()
A = pkg.abi
dev = torch.device("cuda", 0)
SHAPES = {"cora": ([8, 8], [8, 8]), "pubmed": ([8, 8], [8, 8]), "arxiv": ([8, 8, 8], [8, 8, 8])}
LR, B1, B2, EPS, THR = 0.01, 0.9, 0.999, 1e-8, 5.0
VARIANTS = ("a_zero_step_clip_adam", "b_step_optimizer_step", "c_train_step")


def make(ds, d_rp, heads, outdims, variant):
    ctx = pkg.GatContext(heads, outdims, ds["f"], ds["c"])
    ctx.set_graph_device(d_rp.data_ptr(), ds["d_col_idx"].data_ptr(), ds["n"], ds["e"])
    ctx.set_features_device(ds["d_x"].data_ptr(), ds["n"], ds["f"])
    ctx.set_labels_device(ds["d_labels"].data_ptr(), ds["n"])
    ctx.params_init(42)
    if variant != VARIANTS[0]:
        ctx.set_optimizer("adam", LR, betas=(B1, B2), eps=EPS, clip=("group", THR))
    ctx.step_graph(True)
    return ctx


def epoch(ctx, variant, t):
    if variant == VARIANTS[0]:
        ctx.zero_grad(); ctx.step(want_loss=False); ctx.clip(THR); ctx.step_adam(LR, B1, B2, EPS, t)
    elif variant == VARIANTS[1]:
        ctx.zero_grad(); ctx.step(want_loss=False); ctx.optimizer_step()
    else:
        ctx.train_step(want_loss=False)


res = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "optimizer": "Adam, per-group clip at 5, lr 0.01", "workloads": {}}
live = []
try:
    for name in args.workloads.split(","):
        heads, outdims = SHAPES[name]
        ds = pkg.synth.make_dataset_device(name, dev)
        d_rp = torch.from_numpy(np.ascontiguousarray(ds["row_ptr"], np.int32)).to(dev)
        ctxs = {v: make(ds, d_rp, heads, outdims, v) for v in VARIANTS}
        live.append((name, ds, d_rp, ctxs))
        res["workloads"][name] = {"n": ds["n"], "e": ds["e"], "heads": heads, "outdims": outdims, "n_params": ctxs[VARIANTS[0]].n_params,
                                  "runs": {v: {"ms_per_epoch_rounds": []} for v in VARIANTS}}
    counters = {}
    for _ in range(args.rounds):
        for name, ds, d_rp, ctxs in live:
            for v in VARIANTS:
                ctx = ctxs[v]
                t = counters.get((name, v), 0)
                for _ in range(args.warmup):
                    t += 1
                    epoch(ctx, v, t)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    t += 1
                    epoch(ctx, v, t)
                ctx.sync()
                res["workloads"][name]["runs"][v]["ms_per_epoch_rounds"].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 5))
                counters[(name, v)] = t
                assert ctx.step_graph_state() == 2
finally:
    for _, _, _, ctxs in live:
        for ctx in ctxs.values():
            ctx.close()
for name, w in res["workloads"].items():
    for v in VARIANTS:
        r = w["runs"][v]["ms_per_epoch_rounds"]
        w["runs"][v].update(ms_per_epoch=round(statistics.median(r), 5), min=min(r), max=max(r))
    base = w["runs"][VARIANTS[0]]["ms_per_epoch"]
    for v in VARIANTS:
        w["runs"][v]["ratio_to_a"] = round(w["runs"][v]["ms_per_epoch"] / base, 4)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
