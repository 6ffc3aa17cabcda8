"""CPU check of the case list of tests/test_output_head.py (tests/head_cases.py): with the oracle's H_L in place of the
tapped one, every case keeps its undecided nodes under the cap, the saturated cases saturate (and have labels whose
probability underflows), and the tied classes lead on enough nodes — the seeds are chosen so that this holds."""
import numpy as np

import head_cases as hc
import head_ref as hr


def test_cases_are_well_posed(orc):
    names = set()
    for case in hc.BY_NAME.values():
        assert case.name not in names
        names.add(case.name)
        if case.n > 5000:                      # no oracle for the many-tile case: its cap is asserted on the card alone
            continue
        inp = hc.make_inputs(case)
        assert len(inp["ci"]) < 1500
        cfg = orc.Config(list(case.heads), list(case.outdims), case.in_dim, case.C)
        fw = orc.step(cfg, inp["rp"], inp["ci"], inp["lab"], inp["x"], inp["W"], inp["a"], inp["Wo"], backward=False)
        HL = fw.taps["H"][-1]
        hc.finish_inputs(case, inp, HL)        # asserts the saturation / the lead of the tied classes
        ref = hr.head_ref(HL, fw.taps["hpre"][-1], inp["Wo"], inp["lab"], inp["mask"], case.last[0], hc.SLOPE, case.flat)
        assert len(ref.undecided) <= max(2.0, 0.01 * case.n), (case.name, len(ref.undecided))
        if case.wo == "saturated":
            z = hr.logits(HL, inp["Wo"])
            assert 100 <= np.abs(z).max() <= 200
            assert (ref.nll[inp["special"]] == hc.NLL_CLAMPED).all() and (ref.y.astype(np.float32) == 0).any()
        if case.masked:
            assert not inp["mask"][0] and not inp["mask"][-1] and 0.25 < 1 - inp["mask"].mean() < 0.55
            assert not (inp["mask"] & inp["split"]).any()
