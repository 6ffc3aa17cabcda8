#!/usr/bin/env python3
"""sweep.py PARENT_LISTING.s PARENT_LISTING_EXP.s — build pick_sweep.hip with the release flags and with -DGAT_EXPERIMENTS, run each once per
setting of the six choice switches (96 processes: they are read once per process), and report
  1. the inputs compared and the differences found (must be 0), and
  2. the distinct kernels the PARENT's ladders returned over the sweep, per template, against the kernel symbols of those templates in the
     parent's hipcc -S listing of gat_edge_kernels.hip; a symbol no input reached is listed by name.
Needs no GPU.  Writes pick_sweep.txt next to itself."""
import itertools
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "csrc")
FLAGS = ["-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-Wall", "-Wno-unused-function",
         "-munsafe-fp-atomics"]
SWITCHES = {"GAT_ROWGROUP": "01", "GAT_PACKED": "01", "GAT_CPL": "24", "GAT_FWD_WAVES": "124", "GAT_GROUP_MSG": "01", "GAT_STASH_LINES": "01"}
TEMPLATES = ("edge_fwd_kernel", "edge_fwd2_kernel", "edge_fwd3_kernel", "edge_fwd_fix_kernel", "edge_bwd_kernel", "edge_bwd2_kernel",
             "edge_bwd2s_kernel", "edge_bwd3_kernel", "edge_bwd4_kernel")


def template_of(sym):
    m = re.match(r"_ZN3gat12_GLOBAL__N_1\d+(edge_\w+?_kernel)I", sym)
    return m.group(1) if m and m.group(1) in TEMPLATES else None


def run(tag, defs, listing, out):
    exe = os.path.join(tempfile.mkdtemp(), "pick_sweep")
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + defs + [os.path.join(HERE, "pick_sweep.hip"), "-o", exe], check=True)
    names = {}
    for ln in subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout.splitlines():
        addr, _, sym = ln.split(" ", 2) if ln.count(" ") >= 2 else ("", "", "")
        if addr and template_of(sym):
            names[int(addr, 16)] = sym
    env0 = {k: v for k, v in os.environ.items() if not k.startswith("GAT_")}
    inputs = diffs = procs = 0
    reached = set()
    for combo in itertools.product(*SWITCHES.values()):
        r = subprocess.run([exe], env=dict(env0, **dict(zip(SWITCHES, combo))), capture_output=True, text=True)
        procs += 1
        m = re.search(r"SWEEP inputs (\d+) differences (\d+)", r.stdout)
        inputs += int(m.group(1)); diffs += int(m.group(2))
        for ln in r.stdout.splitlines():
            if ln.startswith("DIFF"):
                out.append(f"{tag} {dict(zip(SWITCHES, combo))}: {ln}")
            if ln.startswith("FN "):
                reached.add(names[int(ln.split()[1], 16)])
    listed = {s for s in re.findall(r"\.amdhsa_kernel (\S+)", open(listing).read()) if template_of(s)}
    out.append(f"{tag}: {procs} processes, {inputs} inputs compared, {diffs} differences")
    for t in TEMPLATES:
        out.append(f"{tag}:   {t}: reached {sum(template_of(s) == t for s in reached)}, in the parent's listing {sum(template_of(s) == t for s in listed)}")
    out.append(f"{tag}: distinct kernels the parent's ladders returned {len(reached)}, kernel symbols of the nine templates in the parent's listing {len(listed)}")
    for s in sorted(listed - reached):
        out.append(f"{tag}: NOT REACHED {s}")
    for s in sorted(reached - listed):
        out.append(f"{tag}: NOT IN THE LISTING {s}")
    return diffs == 0 and reached == listed


def main():
    out = []
    ok = run("release", [], sys.argv[1], out)
    ok = run("experiments", ["-DGAT_EXPERIMENTS"], sys.argv[2], out) and ok
    text = "\n".join(out) + "\n"
    open(os.path.join(HERE, "pick_sweep.txt"), "w").write(text)
    sys.stdout.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
