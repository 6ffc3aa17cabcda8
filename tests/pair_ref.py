"""The fp64 autograd model of a training step with a pair head (include/gatv2_abi.h "pair head"): tests/step_ref.py::forward with the
pair head of tests/head_model.py — the last hout X, still attached to the autograd graph, is gathered into the pair rows
    mul:  Q[p] = X[u_p] * X[v_p]        add:  Q[p] = X[u_p] + X[v_p]
and the head of the chosen loss mode (softmax + cross-entropy, MSE, BCE in its smooth form) runs on the P rows.
Also what tests/test_pair_head.py and tests/test_pair_cpu.py share: the pair list, the cases, the seed search, the context builder."""
import functools

import numpy as np

import edge_feat_ref as EF
import head_model as HD
import loss_ref as LR
import readout_ref as RR
import step_ref as SR

MODES = ("mul", "add")
SOFTMAX, BCE, MSE = HD.SOFTMAX, HD.BCE, HD.MSE
Y_MIN = RR.Y_MIN          # a softmax case needs y[label] > Y_MIN for every pair that trains (readout_ref: the model's loss clamp)
FE = RR.FE
D5_FAMILY = RR.D5_FAMILY  # D_last = 5: the scalar-load path of the gather and the scatter
VARIANTS = ("res_norm_reg", "fe3", "mask")
HUB = 7                   # the node of PAIRS with more than 256 incidences (also the graph's hub row)


def gather(X, u, v, mode):
    """X [N][DL] torch -> Q [P][DL] (autograd through X)."""
    import torch
    ui, vi = torch.from_numpy(np.asarray(u)).long(), torch.from_numpy(np.asarray(v)).long()
    return X[ui] * X[vi] if mode == "mul" else X[ui] + X[vi]


def pair_list(n, seed=17, hub=HUB, n_hub=262, n_rand=136):
    """About 400 pairs on n nodes: n_hub pairs with `hub` as u or v in turn (the node carries more than 256 incidences: segments and the
    combine kernel), random pairs, a u == v pair of the hub and one of another node, a pair given twice; node n - 1 is in no pair."""
    rng = np.random.default_rng(seed)
    other = rng.integers(0, n - 1, n_hub)
    u = np.where(np.arange(n_hub) % 2 == 0, hub, other)
    v = np.where(np.arange(n_hub) % 2 == 0, other, hub)
    ru, rv = rng.integers(0, n - 1, n_rand), rng.integers(0, n - 1, n_rand)
    u = np.concatenate([u, ru, [hub, 11, 20, 20]])
    v = np.concatenate([v, rv, [hub, 11, 31, 31]])
    return u.astype(np.int32), v.astype(np.int32)


def forward(cfg, g, u, v, mode, loss, sup, P, mask=None, **kw):
    """fp64 step with a pair head.  g: the graph dict of tests/feature_cases.py (its node labels are not used); u, v [P]; loss: SOFTMAX
    (sup = labels [P]), BCE (smooth form: head_model.loss says why) or MSE (sup = targets [P][C], NaN = missing); mask [P] bool or None
    (pairs outside it: no loss); **kw: step_ref.forward's keywords.  -> the model's dict with loss (over the pairs), y [P][C], paired
    (Q, grad retained) and, for SOFTMAX, loss_per_pair and y_label_min."""
    out = SR.forward(cfg, g["row_ptr"], g["col_idx"], None, g["x"], *P, **kw,
                     head=HD.head("pair_" + mode, loss, sup, mask, u=u, v=v, smooth_bce=True))
    out["paired"] = out["xin"]
    if loss == SOFTMAX:
        keep = np.ones(len(out["y"]), bool) if mask is None else np.asarray(mask, bool)
        out["loss_per_pair"] = out["loss_per_row"]
        out["y_label_min"] = float(out["y"][np.arange(len(keep)), np.asarray(sup)][keep].min())
    return out


# -- the cases of tests/test_pair_head.py, shared with its CPU twin (the seed condition)
def families(FC):
    return list(FC.FAMILIES) + [D5_FAMILY]


def cases(FC):
    """(family name, heads, outdims, GatContext keywords, variant, pair mode, loss)"""
    out = [(n, h, d, kw, "plain", m, SOFTMAX) for n, h, d, kw in families(FC) for m in MODES]
    two = [f for f in FC.FAMILIES if f[0] in ("records_d8", "generic")]
    out += [(n, h, d, kw, "plain", m, l) for n, h, d, kw in two for l in (BCE, MSE) for m in MODES]
    out += [(n, h, d, kw, v, m, SOFTMAX) for n, h, d, kw in two for v in VARIANTS for m in MODES]
    return out


def case_id(case):
    return f"{case[0]}-{case[4]}-{case[5]}-{case[6]}"


def pair_labels(n_pairs, c, seed=31):
    return np.random.default_rng(seed).integers(0, c, n_pairs).astype(np.int32)


def pair_mask(n_pairs, seed=3):
    return LR.row_mask(n_pairs, seed)


def label_prob_min(X, Wo, u, v, mode, labels, mask=None):
    """Smallest y[p][label_p] over the pairs that train, of the softmax head on the pair rows of X (torch fp64, numpy Wo [C][DL])."""
    Q = gather(X.detach(), u, v, mode).numpy()
    z = Q @ np.asarray(Wo, np.float64).T
    ez = np.exp(z - z.max(1, keepdims=True))
    y = ez / (ez.sum(1, keepdims=True) + 1e-8)
    keep = np.ones(len(Q), bool) if mask is None else np.asarray(mask, bool)
    return float(y[np.arange(len(Q)), np.asarray(labels)][keep].min())


def with_clamp(base, u, v, mode, loss, labels, mask=None):
    """The feature's kink predicate `base` plus, for the softmax head, no trained pair at the loss clamp (Y_MIN)."""
    def clear(ref):
        if not base(ref):
            return False
        if loss != SOFTMAX:
            return True
        X = ref["hout"][-1]
        Wo = ref["Wo"].detach().numpy().reshape(-1, X.shape[1])
        return label_prob_min(X, Wo, u, v, mode, labels, mask) > Y_MIN
    return clear


def pick(FC, orc, cfg, g, u, v, mode, loss, labels, mask=None, variant="plain", bf16=False):
    """The parameter seed of a case: the first of 40 whose node model is clear of the LeakyReLU kinks at the bounds of the feature's own
    tests and, for softmax, keeps every trained pair off the loss clamp.  A case without one FAILS (the share of cases the search may
    drop is zero).  -> (W, a, Wo), dict of the other inputs, seed."""
    if variant == "fe3":
        ea = EF.edge_attrs(g, FE)

        def model(ps, P):
            inp = dict(ea=ea, We=SR.xavier_we(cfg, FE, ps))
            return inp, SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, **inp, bf16_pl=bf16)
        P, inp, ref = FC.pick_params(orc, cfg, model, with_clamp(FC.CLEAR_HPRE, u, v, mode, loss, labels, mask))
        return P, inp, ref["seed"]
    if variant == "res_norm_reg":
        P, inp, ref = FC.pick_case(orc, cfg, g, FC.NORM_MODES[1], norm=True, reg=FC.REG, bf16_pl=bf16,
                                   clear=with_clamp(FC.CLEAR_V, u, v, mode, loss, labels, mask))
        return P, inp, ref["seed"]
    P, inp, ref = FC.pick_case(orc, cfg, g, None, bf16_pl=bf16, clear=with_clamp(FC.CLEAR_HPRE, u, v, mode, loss, labels, mask))
    return P, {}, ref["seed"]


@functools.lru_cache(maxsize=None)
def _case_inputs(family, variant, mode, loss, n_rand=None):
    import __graft_entry__ as entry
    import feature_cases as FC
    pkg, orc = entry.load_package(), entry.load_oracle()
    g = FC.parity_graph()
    if loss == BCE:                                  # C = 1: the link-prediction head (the node labels only feed the dummy node head)
        g = dict(g, c=1, labels=np.zeros(g["n"], np.int32))
    _, heads, outdims, kw = next(f for f in families(FC) if f[0] == family)
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    bf16 = kw.get("dtype") == "bf16"
    u, v = pair_list(g["n"]) if n_rand is None else pair_list(g["n"], n_rand=n_rand)
    n_pairs = len(u)
    labels = pair_labels(n_pairs, g["c"])
    if loss == SOFTMAX:
        sup = labels
    elif loss == BCE:
        sup = (np.random.default_rng(41).random((n_pairs, 1)) > 0.5).astype(np.float32)
    else:
        sup = LR.targets_for(pkg, MSE, n_pairs, g["c"])        # NaN holes (loss_ref.MISSING)
    mask = pair_mask(n_pairs) if variant == "mask" else None
    P, inp, seed = pick(FC, orc, cfg, g, u, v, mode, loss, labels, mask, variant, bf16)
    reg = FC.REG if variant == "res_norm_reg" else None
    keeps, attn, feat = FC.masks(cfg, g, cfg.heads, reg)
    return dict(g=g, u=u, v=v, heads=heads, outdims=outdims, kw=kw, cfg=cfg, P=P, inp=inp, seed=seed, sup=sup, mask=mask, loss=loss,
                reg=reg, bf16=bf16, model_kw=dict(eps=FC.EPS, keeps=keeps, attn=attn, feat=feat, bf16_pl=bf16))


def case_inputs(case, n_rand=None):
    """Everything a case runs on (cached: the seed search runs once per process).  case: an entry of cases(); n_rand: the random pairs of
    pair_list (None: its own count), for a longer pair list (tests/trip_cases.py)."""
    key = (case[0], case[4], case[5], case[6])
    return dict(_case_inputs(*key) if n_rand is None else _case_inputs(*key, n_rand), mode=case[5])


def model_of(ci, u=None, v=None):
    """The fp64 model of case_inputs' result (u, v: other pairs of the same length), after loss.backward()."""
    ref = forward(ci["cfg"], ci["g"], ci["u"] if u is None else u, ci["v"] if v is None else v, ci["mode"], ci["loss"], ci["sup"], ci["P"],
                  mask=ci["mask"], **ci["inp"], **ci["model_kw"])
    ref["loss"].backward()
    return ref


def make_ctx(pkg, ci, mode=None, u=None, v=None, **kw):
    """A context of a case with pair mode `mode` (default: the case's; 0 / "none": the call is made with mode 0; False: not made), the
    parameter groups set and the gradients zeroed.  Without a pair head the node labels are set.  **kw goes to GatContext on top of
    the family's keywords."""
    import feature_cases as FC
    A = pkg.abi
    g, inp = ci["g"], ci["inp"]
    ctx = pkg.GatContext(ci["heads"], ci["outdims"], g["f"], g["c"], **dict(ci["kw"], **kw))
    if inp.get("gamma") is not None:
        ctx.set_norm(eps=FC.EPS)
    if inp.get("We") is not None:
        ctx.set_edge_dim(FE)
    if inp.get("Wres") is not None or inp.get("b") is not None:
        ctx.set_residual(linear=inp.get("Wres") is not None, bias=inp.get("b") is not None)
    mode = ci["mode"] if mode is None else mode
    on = mode not in (False, 0, "none")
    if on and ci["loss"] != SOFTMAX:
        ctx.set_loss(ci["loss"])
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    if mode is not False:
        ctx.set_pairs(mode, ci["u"] if u is None else u, ci["v"] if v is None else v)
    if not on:
        ctx.set_labels(g["labels"])
    elif ci["loss"] == SOFTMAX:
        ctx.set_labels(ci["sup"])
    else:
        ctx.set_targets(ci["sup"])
    if inp.get("ea") is not None:
        ctx.set_edge_features(inp["ea"])
    for grp, name in ((A.PARAM_WRES, "Wres"), (A.PARAM_B, "b"), (A.PARAM_LN_G, "gamma"), (A.PARAM_LN_B, "beta"), (A.PARAM_WE, "We")):
        if inp.get(name) is not None:
            ctx.params_set(grp, inp[name])
    for grp, arr in zip((A.PARAM_W, A.PARAM_A, A.PARAM_WO), ci["P"]):
        ctx.params_set(grp, arr)
    if ci["reg"] is not None:
        ctx.set_dropout(ci["reg"]["pf"], ci["reg"]["pa"], seed=ci["reg"]["seed"], first_step=0)
        ctx.set_dropedge(ci["reg"]["pe"])
    if on and ci["mask"] is not None:
        ctx.set_train_mask(ci["mask"])
    ctx.zero_grad()
    return ctx
