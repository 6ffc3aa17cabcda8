"""The dropout / DropEdge, residual / bias and layer-normalisation forms of the edge kernels at every fast-path shape
(include/gatv2_abi.h: "works with every (H, D) family, bf16 storage, keep_taps"): all 14 (H*D, D) shapes of GAT_EDGE_SHAPES x fp32 / bf16
storage x four forms, each one context and one step against the fp64 model of tests/step_ref.py at the project's bars (1e-4 of max-abs
for fp32, 1e-2 for bf16 storage).  tests/test_edge_shapes_cpu.py names the kernel instantiation every case reaches (COVERAGE) and
proves on the host that every case has a parameter seed clear of the LeakyReLU kinks.

A shape (HD, D) is the two-layer model heads [H, H], outdims [D, D], H = HD / D: it runs once as a hidden layer and once as the last.
The graph is parity_graph of tests/feature_cases.py (150 nodes — no multiple of the 16 rows per wave of (8, 4) — 700 edges, a hub row of
300 in-edges processed as segments, one empty row, F = 24, C = 5) and the regularisers are its REG; the case table (SHAPES, DTYPES, FORMS, CASES) is there too."""
import numpy as np
import pytest

import feature_cases as FC
import parity
from feature_cases import CASES, FORMS, REG, case_id

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-4, "bf16": 1e-2}
NORM_RES = FC.NORM_MODES[1]


_REFS = {}


def reference(orc, hd, d, dt, form):
    """The fp64 model of a case after its backward, computed once: the keep_taps form shares the one of res_norm_reg."""
    norm, reg, _ = FORMS[form]
    key = (hd, d, dt, norm, reg)
    if key not in _REFS:
        g, heads, outdims, cfg = FC.shape_model(orc, hd, d)
        out = FC.pick_shape(orc, cfg, g, norm, REG if reg else None, dt == "bf16")
        out[-1]["loss"].backward()
        _REFS[key] = out
    return _REFS[key]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_form_against_fp64(pkg, orc, case):
    """loss / N, every layer's GAT_TAP_HPRE, GAT_TAP_HOUT, GAT_TAP_G and every parameter group of the form (absent groups have size 0)
    at the bar of the storage mode; with keep_taps also GAT_TAP_ALPHA against the model's softmax over the surviving edges, and exact
    zeros in it wherever GAT_TAP_EDGE_KEEP is 0."""
    hd, d, dt, form = case
    norm, reg, taps = FORMS[form]
    A = pkg.abi
    g, heads, outdims, cfg = FC.shape_model(orc, hd, d)
    P, inp, ref = reference(orc, hd, d, dt, form)
    kw = {}
    if dt == "bf16":
        kw["dtype"] = "bf16"
    if taps:
        kw["keep_taps"] = True
    tol = TOL[dt]
    setters = FC.setters(NORM_RES, norm=True) if norm else {}
    with FC.make_ctx(pkg, g, heads, outdims, P, **inp, **setters, reg=REG if reg else None, **kw) as ctx:
        loss, _ = ctx.step()
        FC.compare(pkg, ctx, g, cfg, ref, loss, tol, taps=["hpre", "hout", "G"], groups=FC.GROUPS[:7])
        if taps:
            for l in range(cfg.L):
                want = ref["alpha"][l]
                assert np.abs(want).max() > 0
                got = ctx.tap(A.TAP_ALPHA, l)
                assert got.shape == want.shape
                parity.check_rel(f"alpha[{l}]", got, want, tol)
                keep = ctx.tap(A.TAP_EDGE_KEEP, l) != 0
                assert 0 < keep.sum() < keep.size
                assert np.array_equal(keep, want[0] != 0)        # the model's mask is the device's
                assert (got[:, ~keep] == 0).all()
