"""Writes tests/golden/step_ref_pins.npz: for every form of tests/test_step_ref_cpu.py the loss, s_min, the parameter seed and every
gradient group of the fp64 step model, as float64 under "<form>/<key>".  Run from the repository root:
    python tests/golden/make_step_ref_pins.py
This regenerates the file from tests/step_ref.py itself, which is only right after a deliberate change of the model; the committed file
was written by write() from the four per-feature models step_ref replaced (profiles/step_ref/README.md)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def write(path, forward):
    """forward(form) -> the model to pin that form with (step_ref.forward's signature)."""
    import conftest  # noqa: F401  (puts the repository root on the path)
    import __graft_entry__ as entry
    import test_step_ref_cpu as T
    orc = entry.load_oracle()
    out = {}
    for form in T.FORMS:
        for k, v in T.pin_arrays(orc, form, forward(form)).items():
            out[f"{form}/{k}"] = v
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    import step_ref
    write(os.path.join(HERE, "step_ref_pins.npz"), lambda form: step_ref.forward)
