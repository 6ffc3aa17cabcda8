#!/usr/bin/env python3
"""Cost of the pair head at the Products shape (2.45 M nodes, 61.9 M edges, 2 layers x 8 heads x 8, fp32, D_last = 8): a link-prediction
step — synth.link_pairs with `--pos` positives + `--neg` negatives (2 M + 2 M by default), C = 1, BCE — against the node head with the
same loss IN THE SAME RUN (include/gatv2_abi.h "pair head").  gat_set_pairs sizes the head's buffers, so each setting has a context of
its own; the three (node / mul / add) live in ONE process and run interleaved: `--rounds` passes over the settings, each pass running
`--steps` steps of every setting after `--warmup` untimed ones.  Two passes of their own:
  1. wall clock per step (sync, steps, sync) with collect_timing off — what a training loop sees;
  2. collect_timing on: the head classes' own time per step (HIP-event pairs around every launch, gat_kernel_stats).  The gather is
     timed under head_forward, the scatter under head_backward, together with the head kernels on P rows.
Also the time of one gat_set_pairs_device (check, incidence sort, work list: what a per-epoch resampling of the negatives costs), and
the byte model of the two launches at request granularity: a gathered 32-byte row costs a whole 128-byte request
(gat_request_bytes_shape explains this), streamed arrays cost their bytes.  The two launches' own time is not separable from their
class through gat_kernel_stats where the class holds a head kernel too: gat_step runs the head as ONE fused kernel under head_backward,
so head_forward of a pair context is the gather alone (measured), and the scatter is ESTIMATED as head_backward minus the node context's
head_backward scaled by P / N (the head kernel streams its rows).  The achieved fractions of the 6.3 TB/s practical ceiling are of those
two figures.  Measured, never asserted.
    python tools/pair_cost.py [--workload products] [--scale S] [--pos A] [--neg B] [--steps K] [--warmup W] [--rounds R] [--out profiles/pair_head/cost.json]"""
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
ap.add_argument("--pos", type=int, default=2000000)
ap.add_argument("--neg", type=int, default=2000000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()

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
d_tn = (torch.rand((n, 1), device=dev) < 0.5).float()        # the node head's targets
settings = ["node", "mul", "add"]
HBM = 6.3e12          # practical streaming ceiling (README)
REQ = 128             # bytes of one fabric request
row_req = -(-4 * DL // REQ) * REQ
res = {"workload": args.workload, "scale": args.scale, "n": n, "e": e, "f": f, "c": 1, "loss": "bce", "heads": heads, "outdims": outdims,
       "n_pairs": P, "n_pos": args.pos, "n_neg": args.neg, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
       "runs": {name: {"wall_ms_per_step_rounds": [], "class_ms_rounds": []} for name in settings}}


def build(name, timing):
    ctx = pkg.GatContext(heads, outdims, f, 1, collect_timing=timing)
    ctx.set_loss("bce")
    ctx.set_graph_device(d_rp.data_ptr(), dsd["d_col_idx"].data_ptr(), n, e)
    ctx.set_features_device(dsd["d_x"].data_ptr(), n, f)
    if name == "node":
        ctx.set_targets_device(d_tn.data_ptr(), n, 1)
    else:
        ctx.set_pairs_device(name, d_u.data_ptr(), d_v.data_ptr(), P)
        ctx.set_targets_device(d_t.data_ptr(), P, 1)
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
                res["runs"][name]["algorithmic_bytes_classes"] = per
        if not timing:                                   # one replacement of the pairs: check + incidence sort + work list
            reb = []
            for _ in range(3):
                ctxs["mul"].sync()
                t0 = time.perf_counter()
                ctxs["mul"].set_pairs_device("mul", d_u.data_ptr(), d_v.data_ptr(), P)
                ctxs["mul"].sync()
                reb.append(round((time.perf_counter() - t0) * 1e3, 3))
            res["set_pairs_device_ms"] = reb
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
node = res["runs"]["node"]
for name in ("mul", "add"):
    run = res["runs"][name]
    run["wall_ratio_to_node"] = round(run["wall_ms_per_step"] / node["wall_ms_per_step"], 4)
    # request-granularity bytes of the two launches: gathered rows at whole requests, streams at their bytes
    fwd = 2 * 4 * P + 2 * P * row_req + 4 * P * DL
    bwd = 8 * 2 * P + 2 * P * row_req + (2 * P * row_req if name == "mul" else 0) + 4 * n * DL
    est = {}
    for cls, b in (("head_forward", fwd), ("head_backward", bwd)):
        # (gat_step runs the head as one fused kernel under head_backward: the node context has no head_forward launch, and the pair
        # context's head_forward class is the gather alone)
        own = run["class_ms"].get(cls, 0.0) - node["class_ms"].get(cls, 0.0) * P / n
        est[cls] = {"request_bytes": b, "class_ms": run["class_ms"].get(cls, 0.0), "node_class_ms": node["class_ms"].get(cls, 0.0),
                    "estimated_launch_ms": round(own, 5),
                    "fraction_of_6.3TBps": round(b / (own * 1e-3) / HBM, 4) if own > 0 else None}
    run["launches"] = est
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
