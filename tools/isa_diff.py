#!/usr/bin/env python3
"""isa_diff.py OLD.s NEW.s [--show N] [--pairs FILE] — are two hipcc -S listings the same kernels?

Per kernel: the .amdhsa figures tools/isa_stats.py prints must be equal, and the instruction lines must be equal once comments,
register numbers and local labels are masked ("registers renamed").  "Byte-identical" is the kernel's text as it stands, but for
the number of the function inside its local labels (.LBB<function>_<block>) and the column padding behind such a label, which move when
another kernel is emitted before it.  Kernels whose mangled name exists on one side only are paired
by the longest common prefix of their names (a renamed parameter type changes the tail only) and listed; --pairs FILE pairs by hand
first ("OLD_NAME NEW_NAME" per line: kernels folded into one template, whose names differ in the middle).
Prints one summary line; exit status 1 if any kernel has other differences or stays unpaired."""
import difflib
import re
import sys

FIG = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    s = open(path).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(\S+):[^\n]*@\1\n(.*?)^\.Lfunc_end", s, re.S | re.M)}
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, re.S):
        name, desc = m.group(1), m.group(2)
        out[name] = (bodies[name], tuple(re.search(k + r" (\d+)", desc).group(1) for k in FIG))
    return out


def masked(body):
    lines = []
    for ln in body.splitlines():
        ln = ln.split(";")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        ln = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[R]", ln)
        ln = re.sub(r"\b([vsa])\d+\b", r"\1R", ln)
        lines.append(re.sub(r"\.LBB\d+_\d+", ".L", ln))
    return lines


def unnumbered(body):
    """Local labels, and the comments that cite them, carry the number of their function in the file (.LBB<function>_<block>):
    where a kernel is emitted is not its code.  Nor is the padding between such a label and its comment, which shrinks by a column
    when the function's number gains a digit."""
    return re.sub(r"(?m)^(\.L\w+:)[ \t]+;", r"\1 ;", re.sub(r"(BB|JTI)\d+_(?=\d)", r"\1_", body))


def prefix_len(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def main():
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 40
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pairs = [(n, n) for n in old if n in new]
    lone_old, lone_new = [n for n in old if n not in new], [n for n in new if n not in old]
    if "--pairs" in sys.argv:
        for a, b in (ln.split() for ln in open(sys.argv[sys.argv.index("--pairs") + 1]) if ln.strip()):
            print("paired by hand:", a, "->", b)
            pairs.append((a, b)); lone_old.remove(a); lone_new.remove(b)
    for a in list(lone_old):            # the same kernel under another parameter type: the longest common prefix, both ways
        b = max(lone_new, key=lambda n: prefix_len(a, n), default=None)
        if b is not None and max(lone_old, key=lambda n: prefix_len(n, b)) == a:
            print("renamed:", a, "->", b)
            pairs.append((a, b)); lone_old.remove(a); lone_new.remove(b)
    unpaired = lone_old + lone_new
    for n in unpaired:
        print("unpaired:", n)
    same = renamed = other = 0
    for a, b in pairs:
        (ba, fa), (bb, fb) = old[a], new[b]
        ma, mb = masked(ba), masked(bb)
        if fa == fb and unnumbered(ba) == unnumbered(bb):
            same += 1
        elif fa == fb and ma == mb:
            renamed += 1
        else:
            other += 1
            print("DIFFERS:", b, dict(zip(FIG, fa)) if fa != fb else "", dict(zip(FIG, fb)) if fa != fb else "")
            for ln in list(difflib.unified_diff(ma, mb, "old", "new", n=1, lineterm=""))[:show]:
                print("   ", ln)
    print(f"kernels {len(old)} / {len(new)}: paired {len(pairs)}, byte-identical {same}, registers only renamed {renamed}, "
          f"other differences {other}, unpaired {len(unpaired)}")
    return 1 if other or unpaired else 0


if __name__ == "__main__":
    sys.exit(main())
