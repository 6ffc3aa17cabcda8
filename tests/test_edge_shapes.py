"""The dropout / DropEdge, residual / bias and layer-normalisation forms of the edge kernels at every fast-path shape
(include/gatv2_abi.h: "works with every (H, D) family, bf16 storage, keep_taps"): all 14 (H*D, D) shapes of GAT_EDGE_SHAPES x fp32 / bf16
storage x four forms, each one context and one step against the fp64 model of tests/norm_ref.py at the project's bars (1e-4 of max-abs
for fp32, 1e-2 for bf16 storage).  tests/test_edge_shapes_cpu.py names the kernel instantiation every case reaches (COVERAGE) and
proves on the host that every case has a parameter seed clear of the LeakyReLU kinks.

A shape (HD, D) is the two-layer model heads [H, H], outdims [D, D], H = HD / D: it runs once as a hidden layer and once as the last.
The graph is parity_graph of tests/test_residual.py (150 nodes — no multiple of the 16 rows per wave of (8, 4) — 700 edges, a hub row of
300 in-edges processed as segments, one empty row, F = 24, C = 5) and the regularisers are its REG."""
import itertools

import numpy as np
import pytest

import norm_ref as NR
import parity
import test_norm as TN
from test_residual import REG, masks, parity_graph

pytestmark = pytest.mark.gpu

SHAPES = [(64, 8), (64, 4), (64, 16), (64, 32), (64, 64), (32, 8), (32, 4), (32, 16), (32, 32), (16, 4), (16, 8), (16, 16), (8, 4), (8, 8)]
DTYPES = ["fp32", "bf16"]
# form -> (set_norm + set_residual(linear, bias), the three regularisers of REG, keep_taps)
FORMS = {
    "reg": (False, True, False),
    "res_norm": (True, False, False),
    "res_norm_reg": (True, True, False),
    "taps_res_norm_reg": (True, True, True),
}
CASES = [(hd, d, dt, form) for (hd, d), dt, form in itertools.product(SHAPES, DTYPES, FORMS)]
TOL = {"fp32": 1e-4, "bf16": 1e-2}
NORM_RES = TN.MODES[1]


def case_id(case):
    hd, d, dt, form = case
    return f"hd{hd}_d{d}-{dt}-{form}"


def model(orc, hd, d):
    h = hd // d
    g = parity_graph()
    return g, [h, h], [d, d], orc.Config([h, h], [d, d], g["f"], g["c"])


def pick_params(orc, cfg, g, norm, reg, bf16):
    """First parameter seed (of 40) whose fp64 model needs no kink bookkeeping.  With the norm: tests/test_norm.py::pick_params (norm +
    both residual flags; |s| > 1e-5, |v| > 1e-4).  Without: the plain regularised model, v = h_pre, at the bounds of
    tests/test_residual.py (|s| > 1e-5, |h_pre| > 1e-5).  -> (W, a, Wo), Wres | None, b | None, gamma | None, beta | None, outputs."""
    if norm:
        return TN.pick_params(orc, cfg, g, NORM_RES, reg, bf16=bf16)
    keeps, attn, feat = masks(cfg, g, cfg.heads, reg)
    for ps in range(40):
        P = orc.xavier_params(cfg, ps)
        ref = NR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, keeps=keeps, attn=attn, feat=feat, bf16_pl=bf16)
        if ref["s_min"] > 1e-5 and ref["v_min"] > 1e-5:
            return P, None, None, None, None, ref
    raise AssertionError("no parameter seed clear of the LeakyReLU kink")


_REFS = {}


def reference(orc, hd, d, dt, form):
    """The fp64 model of a case after its backward, computed once: the keep_taps form shares the one of res_norm_reg."""
    norm, reg, _ = FORMS[form]
    key = (hd, d, dt, norm, reg)
    if key not in _REFS:
        g, heads, outdims, cfg = model(orc, hd, d)
        out = pick_params(orc, cfg, g, norm, REG if reg else None, dt == "bf16")
        out[-1]["loss"].backward()
        _REFS[key] = out
    return _REFS[key]


def make_ctx(pkg, g, heads, outdims, P, Wres, b, gamma, beta, norm, reg, **kw):
    if norm:
        return TN.make_ctx(pkg, g, heads, outdims, P, NORM_RES, Wres, b, gamma, beta, REG if reg else None, **kw)
    A = pkg.abi
    ctx = pkg.GatContext(heads, outdims, g["f"], g["c"], **kw)
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    ctx.set_labels(g["labels"])
    for grp, arr in zip((A.PARAM_W, A.PARAM_A, A.PARAM_WO), P):
        ctx.params_set(grp, arr)
    ctx.set_dropout(REG["pf"], REG["pa"], seed=REG["seed"], first_step=0)
    ctx.set_dropedge(REG["pe"])
    ctx.zero_grad()
    return ctx


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_form_against_fp64(pkg, orc, case):
    """loss / N, every layer's GAT_TAP_HPRE, GAT_TAP_HOUT, GAT_TAP_G and every parameter group of the form (absent groups have size 0)
    at the bar of the storage mode; with keep_taps also GAT_TAP_ALPHA against the model's softmax over the surviving edges, and exact
    zeros in it wherever GAT_TAP_EDGE_KEEP is 0."""
    hd, d, dt, form = case
    norm, reg, taps = FORMS[form]
    A = pkg.abi
    g, heads, outdims, cfg = model(orc, hd, d)
    P, Wres, b, gamma, beta, ref = reference(orc, hd, d, dt, form)
    kw = {}
    if dt == "bf16":
        kw["dtype"] = "bf16"
    if taps:
        kw["keep_taps"] = True
    tol = TOL[dt]
    with make_ctx(pkg, g, heads, outdims, P, Wres, b, gamma, beta, norm, reg, **kw) as ctx:
        loss, _ = ctx.step()
        TN.compare(pkg, ctx, g, cfg, ref, loss, tol)
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
