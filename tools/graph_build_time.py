#!/usr/bin/env python
"""tools/graph_build_time.py [--workload products] [--runs 7] [--numpy-flags 0,1,5,6] --out FILE

Time of the device graph builder (gat_graph_from_coo_device, csrc/gat_graph.hip) at a BASELINE shape: the generated CSR is
expanded to an edge list on the device and shuffled with a fixed permutation; every flag set is built warm, `runs` times,
bracketed by device events (the call synchronises its stream, so the events see the whole build including its two host
round-trips), and the median / min / max are reported next to
  - the numpy reference (tests/graph_ref.py) on the same input, on the CPUs this process is granted,
  - the context set-up of the parent (set_graph_device + features + labels: work list and source-major index, bench.py's
    `index_s`) as a scale,
  - the peak temporary device memory of the build (free memory sampled by a second thread while the build runs) and its model
    (16 B x intermediate edges).
Needs the GPU; there is no CPU path."""
import argparse
import json
import math
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = {0: "0", 1: "SELF_LOOPS", 5: "SELF_LOOPS|COALESCE", 6: "SYMMETRIZE|COALESCE"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--numpy-flags", default="0,1,5,6", help="flag sets the numpy reference is timed for ('' = none)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as entry
    from graph_ref import graph_ref
    pkg = entry.load_package()
    A = pkg.abi
    dev = torch.device("cuda:0")
    dsd = pkg.synth.make_dataset_device(args.workload, dev, scale=args.scale)
    n, e, f, c = dsd["n"], dsd["e"], dsd["f"], dsd["c"]
    d_rp = torch.from_numpy(dsd["row_ptr"]).to(dev)
    dst = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), (d_rp[1:] - d_rp[:-1]).long())
    mult = 1_000_003
    while math.gcd(mult, e) != 1:
        mult += 2
    perm = (torch.arange(e, dtype=torch.int64, device=dev) * mult + 12345) % e
    src_p, dst_p = dsd["d_col_idx"][perm].contiguous(), dst[perm].contiguous()
    del perm, dst
    out = {"workload": args.workload, "n_rows": n, "n_in": e, "runs": args.runs, "cpus": len(os.sched_getaffinity(0)),
           "device": torch.cuda.get_device_name(0), "flags": {}}
    for flags in (0, 1, 5, 6):
        m = A.graph_from_coo_device(src_p.data_ptr(), dst_p.data_ptr(), e, n, flags=flags)
        rp = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ci = torch.empty(m, dtype=torch.int32, device=dev)

        def build():
            A.graph_from_coo_device(src_p.data_ptr(), dst_p.data_ptr(), e, n, flags=flags, d_row_ptr=rp.data_ptr(),
                                    d_col_idx=ci.data_ptr(), col_capacity=m)
        build()                                                     # warm: code objects, the sort's algorithm choice
        ms = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); build(); e1.record(); e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        # peak temporary memory: free device memory sampled while one more build runs
        torch.cuda.synchronize()
        free0, low, stop = A.mem_info()[0], [None], threading.Event()

        def sample():
            while not stop.is_set():
                fr = A.mem_info()[0]
                low[0] = fr if low[0] is None else min(low[0], fr)
        t = threading.Thread(target=sample); t.start()
        time.sleep(0.01); build(); stop.set(); t.join()
        slots = e * (2 if flags & 2 else 1) + (n if flags & 1 else 0)
        rec = {"name": NAMES[flags], "edges_out": m, "intermediate_edges": slots, "build_ms_median": ms[len(ms) // 2],
               "build_ms_min_max": [ms[0], ms[-1]], "temp_bytes_model": 16 * slots, "temp_bytes_peak_sampled": free0 - low[0],
               "numpy_s": None}
        out["flags"][str(flags)] = rec
        print(json.dumps(rec), flush=True)
        if str(flags) in args.numpy_flags.split(","):
            s_h, d_h = src_p.cpu().numpy(), dst_p.cpu().numpy()
            t0 = time.perf_counter()
            ref = graph_ref(s_h, d_h, n, flags=flags)
            rec["numpy_s"] = time.perf_counter() - t0
            rec["equal_to_numpy"] = bool(np.array_equal(ref[0], rp.cpu().numpy()) and np.array_equal(ref[1], ci.cpu().numpy()))
            del ref, s_h, d_h
            print(json.dumps({"name": NAMES[flags], "numpy_s": rec["numpy_s"], "equal_to_numpy": rec["equal_to_numpy"]}), flush=True)
        del rp, ci
    # the scale: the context set-up every run pays already (work list + source-major index), as bench.py times `index_s`
    ts = []
    for _ in range(3):
        with pkg.GatContext([8, 8], [8, 8], f, c) as ctx:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.set_graph_device(d_rp.data_ptr(), dsd["d_col_idx"].data_ptr(), n, e)
            ctx.set_features_device(dsd["d_x"].data_ptr(), n, f)
            ctx.set_labels_device(dsd["d_labels"].data_ptr(), n)
            ctx.sync()
            ts.append(time.perf_counter() - t0)
    out["context_setup_s"] = sorted(ts)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({"context_setup_s": out["context_setup_s"]}))


if __name__ == "__main__":
    main()
