"""The fp64 step model of tests/step_ref.py and the heads of tests/head_model.py without a GPU, against what does not share their code:
recorded results of the per-feature models they replaced (tests/golden/step_ref_pins.npz; profiles/step_ref/README.md says where they
came from), and tests/torch_ref.py for the residual term of layer 0 in every row."""
import os

import numpy as np

import feature_cases as FC
import step_ref as SR
import torch_ref

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_ref_pins.npz")
HEADS, OUTDIMS = [4, 2], [4, 8]
FE = 3
GRAPH_PTR = [0, 0, 1, 20, 21, 40]                # an empty graph, two single-node graphs; the mask leaves the last graph out
STATS = ("batch_mean", "batch_rstd", "running_mean", "running_var")
# form -> (the model that runs it: a key of models(), the gradient groups it has).  The first six are the forms of the first fold (the
# four per-feature layer models), the others those of the second (edge term, batch norm, the heads).
FORMS = {
    "plain": ("step", 3), "keeps_attn_feat": ("step", 3), "res_flat": ("step", 5), "norm_res_reg": ("step", 7),
    "norm_res_skip_last": ("step", 7), "norm_res_reg_bf16": ("step", 7),
    "edge_plain": ("edge", 4), "edge_norm_res_reg": ("edge", 8), "edge_bf16": ("edge", 4),
    "bn_train": ("bn", 6), "bn_eval": ("bn", 7), "bn_skip_last": ("bn", 7),
    "readout_mean": ("readout", 3), "readout_sum": ("readout", 3), "readout_max": ("readout", 3),
    "pair_mul_softmax": ("pair", 3), "pair_mul_bce": ("pair", 3), "pair_mul_mse": ("pair", 3),
    "pair_add_softmax": ("pair", 3), "pair_add_bce": ("pair", 3), "pair_add_mse": ("pair", 3),
    "node_bce": ("loss", 3), "node_mse": ("loss", 3),
    "hidden_relu_node": ("hidden", 5), "hidden_relu_readout": ("hidden", 5), "hidden_relu_pair_mul": ("hidden", 5),
    "hidden_lrelu_node": ("hidden", 5), "hidden_lrelu_readout": ("hidden", 5), "hidden_lrelu_pair_add": ("hidden", 5),
}


def models():
    """What runs each kind of form today.  (tests/golden/make_step_ref_pins.py::write was given the replaced models in these places.)"""
    import head_mlp_ref
    import loss_ref
    import pair_ref
    import readout_ref
    return dict(step=SR.forward, edge=SR.forward, bn=SR.forward, readout=readout_ref.forward, pair=pair_ref.forward, loss=loss_ref.forward,
                hidden=head_mlp_ref.forward)


def pin_case(orc, c=None):
    g = FC.host_graph(1)
    assert g["n"] == 40 and g["row_ptr"][8] - g["row_ptr"][7] == 40 and g["row_ptr"][3] == g["row_ptr"][4]
    return g, orc.Config(HEADS, OUTDIMS, g["f"], g["c"] if c is None else c)


def pin_kwargs(cfg, g, form, ps):
    """The optional arguments of a pinned form of the layer model at parameter seed ps (masks: the regularisers REG at step 1)."""
    keeps, attn, feat = FC.masks(cfg, g, HEADS, FC.REG)
    Wres, b = SR.xavier_wres(cfg, ps)
    gamma, beta = SR.ln_params(cfg, ps)
    reg = dict(keeps=keeps, attn=attn, feat=feat)
    res = dict(Wres=Wres, b=b)
    norm = dict(res, gamma=gamma, beta=beta, eps=FC.EPS)
    edge = dict(ea=np.random.default_rng(77).standard_normal((len(g["col_idx"]), FE)).astype(np.float32), We=SR.xavier_we(cfg, FE, ps))
    rng = np.random.default_rng(5)
    n = SR.ln_offsets(cfg)[-1]
    running = (rng.uniform(-1, 1, n), rng.uniform(0.5, 2, n))
    return {
        "plain": {},
        "keeps_attn_feat": reg,
        "res_flat": dict(res, flat_lrelu_index=True),
        "norm_res_reg": dict(norm, **reg),
        "norm_res_skip_last": dict(norm, skip_last=True),
        "norm_res_reg_bf16": dict(norm, **reg, bf16_pl=True),
        "edge_plain": edge,
        "edge_norm_res_reg": dict(norm, **reg, **edge),
        "edge_bf16": dict(edge, bf16_pl=True),
        # (no b: the bias gradient of a batch-normalised layer is a sum that vanishes identically, rounding and nothing to pin)
        "bn_train": dict(Wres=Wres, gamma=gamma, beta=beta, eps=FC.EPS, bn=True, momentum=0.1),
        "bn_eval": dict(norm, bn=True, running=running, training=False),
        "bn_skip_last": dict(norm, bn=True, momentum=0.1, skip_last=True),
    }[form]


def _supervision(rows, c, loss, rng):
    """labels (softmax), 0 / 1 targets (BCE) or normal targets (MSE), the last two with a fifth of the entries missing; and a row mask."""
    if loss == "softmax":
        sup = rng.integers(0, c, rows)
    else:
        sup = ((rng.random((rows, c)) > 0.5) if loss == "bce" else rng.standard_normal((rows, c))).astype(np.float32)
        sup[rng.random((rows, c)) < 0.2] = np.nan
    mask = rng.random(rows) > 0.3
    mask[0] = True
    return sup, mask


def run_form(orc, form, M, ps):
    """-> the outputs of a form's model at parameter seed ps.  M: models(), or the replaced models under the same keys."""
    kind = FORMS[form][0]
    parts = form.split("_")
    loss = parts[-1] if kind in ("pair", "loss") else "softmax"
    g, cfg = pin_case(orc, 1 if loss == "bce" and kind == "pair" else None)        # pair BCE: C = 1, the link-prediction head
    P = orc.xavier_params(cfg, ps)
    if kind in ("step", "edge", "bn"):
        return M[kind](cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, **pin_kwargs(cfg, g, form, ps))
    import head_mlp_ref as HM
    import pair_ref as PR
    rng = np.random.default_rng(len(form))
    u, v = PR.pair_list(g["n"], n_hub=20, n_rand=12)
    if kind == "readout":
        gmask = np.array([True, True, True, True, False])
        return M[kind](cfg, g, GRAPH_PTR, parts[1], rng.integers(0, cfg.num_classes, 5), P, gmask=gmask)
    if kind == "pair":
        sup, mask = _supervision(len(u), cfg.num_classes, loss, rng)
        return M[kind](cfg, g, u, v, parts[1], loss, sup, P, mask=mask)
    if kind == "loss":
        sup, mask = _supervision(g["n"], cfg.num_classes, loss, rng)
        return M[kind](cfg, g, sup, loss, P, mask=mask)
    hk = "_".join(parts[2:])                                                         # node, readout, pair_mul, pair_add
    rows = {"node": g["n"], "readout": 5}.get(hk, len(u))
    sup, mask = _supervision(rows, cfg.num_classes, "softmax", rng)
    W1, b1, Wo = HM.head_values(OUTDIMS[-1], 6, cfg.num_classes)
    return M[kind](cfg, g, hk, "softmax", sup, P[:2], W1, b1, Wo, parts[1], mask=mask, graph_ptr=GRAPH_PTR if hk == "readout" else None,
                   u=u if hk.startswith("pair") else None, v=v if hk.startswith("pair") else None)


def pin_arrays(orc, form, M):
    """-> {key: float64 array} of a form: loss, s_min, every gradient group, the four statistics of a batch-norm form and y of a head
    form, at the first of 40 parameter seeds that keeps |s|, |h_pre| and |v| above 1e-5 (last-bit differences between hosts then change
    no LeakyReLU branch)."""
    clear = FC.clear_of(s=1e-5, hpre=1e-5, v=1e-5)
    for ps in range(40):
        ref = run_form(orc, form, M, ps)
        if clear(ref):
            break
    else:
        raise AssertionError("no parameter seed clear of the LeakyReLU kink")
    ref["loss"].backward()
    out = {"loss": np.float64(ref["loss"].item()), "s_min": np.float64(ref["s_min"]), "seed": np.float64(ps)}
    for k in FC.GROUPS:
        if ref.get(k) is not None:
            out[f"grad_{k}"] = ref[k].grad.numpy().astype(np.float64)
    kind = FORMS[form][0]
    if kind == "bn":
        out.update({k: np.asarray(ref[k], np.float64) for k in STATS})
    if kind in ("readout", "pair", "loss", "hidden"):
        out["y"] = np.asarray(ref["y"], np.float64)
    return out


def test_the_model_reproduces_the_recorded_results_of_the_models_it_replaced(orc):
    pins = np.load(PINS)
    assert sorted({k.split("/")[0] for k in pins.files}) == sorted(FORMS)
    M = models()
    for form, (kind, groups) in FORMS.items():
        want = {k[len(form) + 1:]: pins[k] for k in pins.files if k.startswith(form + "/")}
        got = pin_arrays(orc, form, M)
        extra = 4 if kind == "bn" else 0 if kind in ("step", "edge") else 1
        assert sorted(got) == sorted(want) and len(want) == 3 + groups + extra, form
        assert got.pop("seed") == want.pop("seed"), form
        for k in want:
            scale = np.abs(want[k]).max()
            assert got[k].shape == want[k].shape, (form, k)
            assert scale > 0 or (form == "bn_eval" and k.startswith("batch_") and not got[k].any()), (form, k)      # eval: no batch statistics
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
