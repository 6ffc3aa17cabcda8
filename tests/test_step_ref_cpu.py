"""The fp64 step model of tests/step_ref.py without a GPU, against what does not share its code: recorded results of the four
per-feature models it replaced (tests/golden/step_ref_pins.npz; profiles/step_ref/README.md says where they came from), and
tests/torch_ref.py for the residual term of layer 0 in every row."""
import os

import numpy as np

import feature_cases as FC
import step_ref as SR
import torch_ref

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_ref_pins.npz")
HEADS, OUTDIMS = [4, 2], [4, 8]
FORMS = ["plain", "keeps_attn_feat", "res_flat", "norm_res_reg", "norm_res_skip_last", "norm_res_reg_bf16"]


def pin_case(orc):
    g = FC.host_graph(1)
    assert g["n"] == 40 and g["row_ptr"][8] - g["row_ptr"][7] == 40 and g["row_ptr"][3] == g["row_ptr"][4]
    return g, orc.Config(HEADS, OUTDIMS, g["f"], g["c"])


def pin_kwargs(cfg, g, form, ps):
    """The optional arguments of a pinned form at parameter seed ps (masks: the regularisers REG at step 1)."""
    keeps, attn, feat = FC.masks(cfg, g, HEADS, FC.REG)
    Wres, b = SR.xavier_wres(cfg, ps)
    gamma, beta = SR.ln_params(cfg, ps)
    reg = dict(keeps=keeps, attn=attn, feat=feat)
    res = dict(Wres=Wres, b=b)
    norm = dict(res, gamma=gamma, beta=beta, eps=FC.EPS)
    return {
        "plain": {},
        "keeps_attn_feat": reg,
        "res_flat": dict(res, flat_lrelu_index=True),
        "norm_res_reg": dict(norm, **reg),
        "norm_res_skip_last": dict(norm, skip_last=True),
        "norm_res_reg_bf16": dict(norm, **reg, bf16_pl=True),
    }[form]


def pin_arrays(orc, form, forward):
    """-> {key: float64 array} of a form: loss, s_min and every gradient group, at the first of 40 parameter seeds that keeps |s|,
    |h_pre| and |v| above 1e-5 (last-bit differences between hosts then change no LeakyReLU branch).  forward: the model, with
    step_ref.forward's signature."""
    g, cfg = pin_case(orc)
    clear = FC.clear_of(s=1e-5, hpre=1e-5, v=1e-5)
    _, ref = FC.pick_params(orc, cfg, lambda ps, P: (forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P,
                                                             **pin_kwargs(cfg, g, form, ps)),), clear)
    ref["loss"].backward()
    out = {"loss": np.float64(ref["loss"].item()), "s_min": np.float64(ref["s_min"]), "seed": np.float64(ref["seed"])}
    for k in FC.GROUPS:
        if ref[k] is not None:
            out[f"grad_{k}"] = ref[k].grad.numpy().astype(np.float64)
    return out


def test_the_model_reproduces_the_recorded_results_of_the_models_it_replaced(orc):
    pins = np.load(PINS)
    assert sorted({k.split("/")[0] for k in pins.files}) == sorted(FORMS)
    for form in FORMS:
        want = {k[len(form) + 1:]: pins[k] for k in pins.files if k.startswith(form + "/")}
        got = pin_arrays(orc, form, SR.forward)
        groups = {"plain": 3, "keeps_attn_feat": 3, "res_flat": 5}.get(form, 7)
        assert sorted(got) == sorted(want) and len(want) == 3 + groups, form
        assert got.pop("seed") == want.pop("seed"), form
        for k in want:
            scale = np.abs(want[k]).max()
            assert scale > 0 and got[k].shape == want[k].shape, (form, k)
            assert np.abs(got[k] - want[k]).max() <= 1e-12 * scale, (form, k)


def test_layer_0_differs_from_the_plain_model_by_the_residual_term_in_every_row(orc):
    """h_pre of layer 0 with Wres and b, minus h_pre of layer 0 of tests/torch_ref.py (no such term), is x Wres_0^T + b_0: in the empty
    row, where it stands alone, and in every other."""
    g, cfg = pin_case(orc)
    P = orc.xavier_params(cfg, 1)
    Wres, b = SR.xavier_wres(cfg, 1)
    wo, bo = SR.res_offsets(cfg)
    got = FC.run_model(cfg, g, P, Wres=Wres, b=b)["hpre"][0].detach().numpy().reshape(g["n"], -1)
    plain = torch_ref.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P)["hpre"][0].detach().numpy().reshape(g["n"], -1)
    want = g["x"].astype(np.float64) @ Wres[:wo[1]].astype(np.float64).reshape(16, g["f"]).T + b[:bo[1]]
    assert np.abs(plain).max() > 0 and np.abs(want).max() > 0.1
    assert np.abs((got - plain) - want).max() <= 1e-12
