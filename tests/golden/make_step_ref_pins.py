"""Writes tests/golden/step_ref_pins.npz: for every form of tests/test_step_ref_cpu.py the loss, s_min, the parameter seed, every
gradient group, the batch-norm statistics and the head's y of the fp64 step model, as float64 under "<form>/<key>".  Run from the
repository root:
    python tests/golden/make_step_ref_pins.py
This regenerates the file from tests/step_ref.py and its wrappers themselves, which is only right after a deliberate change of the model;
the committed file was written by write() from the per-feature models they replaced, six forms by the first fold and the others, on top
of those (base=), by the second (profiles/step_ref/README.md)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def write(path, models, forms=None, base=None):
    """models: the functions to pin with, under the keys of test_step_ref_cpu.models().  forms: the forms to write (default: all), on
    top of the arrays of base (an earlier file's)."""
    import conftest  # noqa: F401  (puts the repository root on the path)
    import __graft_entry__ as entry
    import test_step_ref_cpu as T
    orc = entry.load_oracle()
    out = dict(base or {})
    for form in forms or T.FORMS:
        for k, v in T.pin_arrays(orc, form, models).items():
            out[f"{form}/{k}"] = v
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    import test_step_ref_cpu
    write(os.path.join(HERE, "step_ref_pins.npz"), test_step_ref_cpu.models())
