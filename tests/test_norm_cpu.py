"""Layer normalisation without a GPU (include/gatv2_abi.h "layer normalisation"): the new ABI symbols, the fp64 model of
tests/step_ref.py against a hand formula and against central differences (tests/test_step_ref_cpu.py pins it against the models it
replaced), the train_edge flags, and — a condition, not a skip — a parameter seed clear of the LeakyReLU kinks for every case tests/test_norm.py runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import feature_cases as T
import step_ref as SR
from feature_cases import host_graph as _graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")


def _run(cfg, g, P, **kw):
    return T.run_model(cfg, g, P, **kw)


def test_symbols_declared_and_exported(pkg):
    A = pkg.abi
    assert "gat_set_norm" in A.declared_symbols()
    assert hasattr(ctypes.CDLL(A.LIB_PATH), "gat_set_norm")
    assert (A.PARAM_LN_G, A.PARAM_LN_B) == (5, 6)
    assert (A.NORM_LAYER, A.NORM_SKIP_LAST) == (1, 2)
    assert A.load_library().gat_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "gatv2_abi.h")).read()
    assert "#define GAT_ABI_VERSION 6" in hdr
    assert "GAT_PARAM_LN_G = 5, GAT_PARAM_LN_B = 6" in hdr and "GAT_NORM_LAYER = 1, GAT_NORM_SKIP_LAST = 2" in hdr
    assert "int gat_set_norm(gat_ctx* ctx, int32_t flags, float eps);" in hdr
    assert hasattr(pkg.GatContext, "set_norm")


def test_one_row_against_the_hand_formula(orc):
    """gamma = 1, beta = 0: hout of a row is LReLU((u - mean u) / sqrt(var + eps)), and with eps -> large it tends to
    LReLU((u - mean u) / sqrt(eps)): the variance no longer matters."""
    g = _graph(1)
    cfg = orc.Config([4, 2], [4, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    n = SR.ln_offsets(cfg)[-1]
    row = 11
    lrelu = lambda t: np.where(t > 0, t, 0.01 * t)
    for eps in (1e-5, 1e6):
        ref = _run(cfg, g, P, gamma=np.ones(n), beta=np.zeros(n), eps=eps)
        u = ref["hpre"][0][row].detach().numpy().reshape(-1)
        assert np.abs(u).max() > 0
        d = u - u.sum() / 16
        want = lrelu(d / np.sqrt((d * d).sum() / 16 + eps))
        got = ref["hout"][0][row].detach().numpy()
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
        if eps == 1e6:
            assert np.abs(got - lrelu(d / 1e3)).max() <= 1e-6 * np.abs(got).max()


def test_empty_row_without_residual_has_v_equal_beta(orc):
    g = _graph(2)
    cfg = orc.Config([4, 2], [4, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 1)
    gamma, beta = SR.ln_params(cfg, 1)
    ref = _run(cfg, g, P, gamma=gamma, beta=beta)
    assert g["row_ptr"][3] == g["row_ptr"][4]
    assert (ref["hpre"][0][3] == 0).all()
    b0 = beta[:16].astype(np.float64)
    assert np.abs(ref["hout"][0][3].detach().numpy() - np.where(b0 > 0, b0, 0.01 * b0)).max() < 1e-15


def test_autograd_matches_central_differences(orc):
    g = _graph(4, n=25, e=120)
    cfg = orc.Config([2, 2], [3, 4], g["f"], g["c"])
    P = orc.xavier_params(cfg, 2)
    Wres, b = SR.xavier_wres(cfg, 2)
    for ps in range(40):
        gamma, beta = (v.astype(np.float64) for v in SR.ln_params(cfg, ps))
        ref = _run(cfg, g, P, Wres=Wres, b=b, gamma=gamma, beta=beta)
        if ref["s_min"] > 1e-4 and ref["v_min"] > 1e-4:      # the probes below stay on one side of every kink
            break
    else:
        raise AssertionError("no gamma / beta seed clear of the LeakyReLU kink")
    ref["loss"].backward()
    rng = np.random.default_rng(0)
    h = 1e-6
    for name, base in (("gamma", gamma), ("beta", beta), ("b", b.astype(np.float64))):
        grad = ref[name].grad.numpy()
        assert np.abs(grad).max() > 0
        for i in rng.choice(base.size, 10, replace=False):
            up, dn = base.copy(), base.copy()
            up[i] += h; dn[i] -= h
            kw = dict(Wres=Wres, b=b, gamma=gamma, beta=beta)
            lu = _run(cfg, g, P, **dict(kw, **{name: up}))["loss"].item()
            ld = _run(cfg, g, P, **dict(kw, **{name: dn}))["loss"].item()
            fd = (lu - ld) / (2 * h)
            assert abs(fd - grad[i]) <= 1e-6 * max(1.0, np.abs(grad).max()), (name, i, fd, grad[i])


def test_the_contracts_backward_formulas_are_autograd(orc):
    """G, grad_gamma and grad_beta as gatv2_abi.h states them (from u, dL/dhout, gamma, beta alone: what the N-sized backward kernel
    reads) against autograd, for a hidden layer (dL/dhout = g) and the last one (dL/dhout = gH / H)."""
    g = _graph(4, n=25, e=120)
    cfg = orc.Config([2, 2], [3, 4], g["f"], g["c"])
    P = orc.xavier_params(cfg, 2)
    Wres, b = SR.xavier_wres(cfg, 2)
    gamma, beta = (v.astype(np.float64) for v in SR.ln_params(cfg, 2))
    eps, slope = 1e-5, 0.01
    ref = _run(cfg, g, P, Wres=Wres, b=b, gamma=gamma, beta=beta, eps=eps)
    ref["loss"].backward()
    o = SR.ln_offsets(cfg)
    for l in range(2):
        H, D = cfg.heads[l], cfg.outdims[l]
        u = ref["hpre"][l].detach().numpy().reshape(g["n"], H * D)
        go = ref["hout"][l].grad.numpy()
        if l == 1:                                               # mean over heads: every head gets gH / H
            go = np.tile(go / H, (1, H))
        gm, bt = gamma[o[l]:o[l + 1]], beta[o[l]:o[l + 1]]
        mu = u.mean(1, keepdims=True)
        rstd = 1 / np.sqrt(((u - mu) ** 2).mean(1, keepdims=True) + eps)
        xhat = (u - mu) * rstd
        dv = go * np.where(gm * xhat + bt > 0, 1.0, slope)
        dxh = dv * gm
        G = rstd * (dxh - dxh.mean(1, keepdims=True) - xhat * (dxh * xhat).mean(1, keepdims=True))
        want = ref["hpre"][l].grad.numpy().reshape(g["n"], H * D)
        assert np.abs(want).max() > 0
        assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max(), l
        assert np.abs((dv * xhat).sum(0) - ref["gamma"].grad.numpy()[o[l]:o[l + 1]]).max() <= 1e-12 * np.abs(ref["gamma"].grad.numpy()).max()
        assert np.abs(dv.sum(0) - ref["beta"].grad.numpy()[o[l]:o[l + 1]]).max() <= 1e-12 * np.abs(ref["beta"].grad.numpy()).max()
        assert np.abs(G.sum(0) - ref["b"].grad.numpy()[o[l]:o[l + 1]]).max() <= 1e-12 * np.abs(ref["b"].grad.numpy()).max()


def test_skip_last_leaves_the_last_entries_without_gradient(orc):
    g = _graph(4, n=25, e=120)
    cfg = orc.Config([2, 2], [3, 4], g["f"], g["c"])
    P = orc.xavier_params(cfg, 2)
    gamma, beta = SR.ln_params(cfg, 2)
    ref = _run(cfg, g, P, gamma=gamma, beta=beta, skip_last=True)
    ref["loss"].backward()
    o = SR.ln_offsets(cfg)
    for k in ("gamma", "beta"):
        assert (ref[k].grad[o[1]:] == 0).all() and ref[k].grad[:o[1]].abs().max() > 0


def test_train_edge_help_lists_the_flags():
    out = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert "--layer-norm" in out.stdout and "--norm-eps" in out.stdout and "--norm-skip-last" in out.stdout


# the (heads, outdims, bf16) the parity cases of tests/test_norm.py run on its graph
GPU_SHAPES = [
    ([8, 8], [8, 8], False), ([16, 16], [4, 4], False), ([4, 4], [16, 16], False), ([2, 2], [8, 8], False), ([3, 2], [5, 8], False),
    ([16, 2], [8, 8], False), ([8, 8], [8, 8], True), ([8, 8, 8], [8, 8, 8], False),
]


@pytest.mark.parametrize("heads,outdims,bf16", GPU_SHAPES,
                         ids=[f"{'x'.join(map(str, h))}_{'x'.join(map(str, d))}{'_bf16' if b else ''}" for h, d, b in GPU_SHAPES])
def test_some_of_the_first_40_seeds_is_clear_of_the_kink(orc, heads, outdims, bf16):
    """The GPU tests pick the first parameter seed with min |s| above 1e-5 and min |v| above 1e-4; the reference alone must offer one
    among the first 40, for every case they run (pick_case of tests/feature_cases.py raises otherwise): norm only and norm + both residual flags, plain and
    with the three regularisers on, and the skip_last case."""
    g = T.parity_graph()
    assert int(g["row_ptr"][8] - g["row_ptr"][7]) == 300 and g["row_ptr"][3] == g["row_ptr"][4]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    for mode in T.NORM_MODES:
        for reg in (None, T.REG):
            T.pick_case(orc, cfg, g, mode, norm=True, reg=reg, bf16_pl=bf16)
    if heads == [8, 8] and not bf16:
        T.pick_case(orc, cfg, g, T.NORM_MODES[1], norm=True, skip_last=True)
        for mode in T.NORM_MODES:
            T.pick_case(orc, cfg, g, mode, norm=True, keeps=T.rows_keeps(g))


def test_the_wide_shapes_have_a_seed_too(orc):
    g = T.wide_graph()
    assert g["row_ptr"][3] == g["row_ptr"][4]
    for _, heads, outdims in T.WIDE:
        T.pick_case(orc, orc.Config(heads, outdims, g["f"], g["c"]), g, T.NORM_MODES[1], norm=True)
