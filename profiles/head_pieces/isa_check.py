#!/usr/bin/env python3
"""isa_check.py OLD.s NEW.s [NEW2.s ...] — check (c) of profiles/head_pieces/README.md for one source that was split.

The kernels of OLD.s (hipcc -S --cuda-device-only) are looked up in the NEW listings together and paired by their demangled name
without the parameter list (the merged argument struct changes the mangled tail only).  Per kernel: byte-identical (tools/isa_diff.py's
notion), or else the .amdhsa figures and the counts of the floating-point multiply / add / fma instructions, old against new.
Exit status 1 if a kernel stays unpaired, or a figure or a count differs."""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tools"))
import isa_diff  # noqa: E402

OPS = ("v_mul_f32", "v_pk_mul_f32", "v_add_f32", "v_pk_add_f32", "v_fmac_f32", "v_fma_f32", "v_pk_fma_f32")


def base_names(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {n: re.sub(r"^void ", "", d).rsplit("(", 1)[0] for n, d in zip(names, out)}


def mix(body):
    c = collections.Counter()
    for ln in body.splitlines():
        op = ln.split(";")[0].split()
        if op and (op[0].split("_e")[0] in OPS or re.match(r"v_\w+_f64", op[0])):
            c[op[0].split("_e")[0]] += 1
    return c


def main():
    old = isa_diff.kernels(sys.argv[1])
    new = {}
    for p in sys.argv[2:]:
        new.update(isa_diff.kernels(p))
    bo, bn = base_names(list(old)), base_names(list(new))
    by_base = {b: n for n, b in bn.items()}
    bad = same = 0
    for n in sorted(old, key=bo.get):
        m = by_base.pop(bo[n], None)
        if m is None:
            print("UNPAIRED (old):", bo[n]); bad += 1
            continue
        (ba, fa), (bb, fb) = old[n], new[m]
        if fa == fb and isa_diff.unnumbered(ba) == isa_diff.unnumbered(bb):
            same += 1
            continue
        ma, mb = mix(ba), mix(bb)
        ops = {k: (ma[k], mb[k]) for k in sorted(set(ma) | set(mb)) if ma[k] != mb[k]}
        verdict = "figures and instruction mix equal" if fa == fb and not ops else "DIFFERS"
        bad += verdict == "DIFFERS"
        print(f"{bo[n]}: {verdict}; vgpr/sgpr/scratch/lds {'/'.join(fa)} -> {'/'.join(fb)}; mix "
              + (" ".join(f"{k}={v}" for k, v in sorted(ma.items())) if not ops else " ".join(f"{k} {a}->{b}" for k, (a, b) in ops.items())))
    for b in by_base:
        print("UNPAIRED (new):", b); bad += 1
    print(f"kernels {len(old)} / {len(new)}: byte-identical {same}, listed above {len(old) - same}, failing {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
