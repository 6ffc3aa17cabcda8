#!/usr/bin/env python3
"""compare_outputs.py LABEL A.npz B.npz — the arrays of two dump_outputs.py runs by bytes.  Prints one line; exit status 1 if they differ."""
import sys

import numpy as np

label, a, b = sys.argv[1], np.load(sys.argv[2]), np.load(sys.argv[3])
keys = sorted(set(a.files) | set(b.files))
bad = [k for k in keys if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
       or a[k].tobytes() != b[k].tobytes()]
cases = len({k.rsplit("/", 1)[0] for k in keys})
print(f"{label}: {cases} cases, {len(keys)} arrays, {len(keys) - len(bad)} byte-identical, {len(bad)} differ", flush=True)
for k in bad[:40]:
    if k in a.files and k in b.files and a[k].shape == b[k].shape:
        d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
        print(f"   DIFFERS {k}: max |a - b| = {np.nanmax(d):.3e}, max |a| = {np.nanmax(np.abs(a[k])):.3e}")
    else:
        print(f"   DIFFERS {k}: missing on one side or another shape")
sys.exit(1 if bad else 0)
