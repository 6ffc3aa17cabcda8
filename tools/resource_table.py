"""Turn hipcc's -Rpass-analysis=kernel-resource-usage remarks (stderr of a compile, saved to a file) into a markdown table:
kernel, VGPRs, AGPRs, scratch bytes per lane, occupancy.  --match keeps the kernels whose demangled name contains the text.

    hipcc ... -Rpass-analysis=kernel-resource-usage -c gat_edge_kernels.hip -o /dev/null 2> remarks.txt
    python tools/resource_table.py remarks.txt --match edge_bwd3_kernel
"""
import argparse
import re
import subprocess


def parse(path):
    rows, cur = [], None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill): (\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "Function Name":
            cur = {"name": val}
            rows.append(cur)
        elif cur is not None:
            cur[key.split(" ")[0] + ("Spill" if key.endswith("Spill") else "")] = int(val)
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    for r, n in zip(rows, names):
        n = re.sub(r"gat::\(anonymous namespace\)::", "", n)
        r["name"] = re.sub(r"\(.*$", "", re.sub(r"^void ", "", n))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("remarks")
    ap.add_argument("--match", action="append", default=[])
    a = ap.parse_args()
    print("| kernel | VGPRs | AGPRs | scratch B/lane | VGPR spills | waves/SIMD |")
    print("|---|---|---|---|---|---|")
    for r in parse(a.remarks):
        if a.match and not any(m in r["name"] for m in a.match):
            continue
        print(f"| `{r['name']}` | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('ScratchSize')} | {r.get('VGPRsSpill')} | {r.get('Occupancy')} |")


if __name__ == "__main__":
    main()
