"""The fp64 autograd model of a training step with a hidden layer in front of the output head (include/gatv2_abi.h "hidden layer"):
tests/step_ref.py::forward with the head of tests/head_model.py on the rows the head reads — hout of the last layer, the pooled rows, the
pair rows — and its hidden layer:
    A = Xin W1^T,   Z1 = act(A + b1),   z = Z1 Wo^T  (Wo [C][Dh])
and the loss of the case run on top.  Also what tests/test_head_mlp.py and tests/test_head_mlp_cpu.py share: the cases, the test values
of W1 / b1 / Wo, the seed search, the context builder."""
import functools

import numpy as np

import edge_feat_ref as EF
import head_model as HD
import loss_ref as LR
import pair_ref as PR
import readout_ref as RR
import step_ref as SR

KINDS = HD.KINDS
SOFTMAX, BCE, MSE = PR.SOFTMAX, PR.BCE, PR.MSE
ACTS = ("relu", "lrelu")
Y_MIN = RR.Y_MIN                  # a softmax case needs y[label] > Y_MIN for every row that trains (readout_ref: the model's loss clamp)
A_MIN = 1e-5                      # every |A + b1| entry above this: the bound CLEAR_HPRE puts on h_pre, so that no kink correction is ever
                                  # applied.  The bound sits on the activation's ARGUMENT A + b1, where the kink of act(A + b1) is — not
                                  # on A = Xin W1^T: b1 is drawn non-zero, so |A| says nothing about the kink, and with MUL pairs (entries
                                  # of Q are products of two small numbers, |A| ~ 0.03) a few of the R * Dh entries of A lie below 1e-5 under
                                  # practically every seed, which would leave those cases without a seed (none may be dropped)
FE = RR.FE
D5_FAMILY = RR.D5_FAMILY
GRAPH_PTR = RR.GRAPH_PTR
VARIANTS = ("res_norm_reg", "fe3", "mask", "keep_taps", "bf16")


def head_values(d_last, dh, c, seed=0):
    """Test values of the stage: W1 [Dh][D_last] Xavier-uniform (lim = sqrt(6 / (D_last + Dh))), b1 ~ U(-0.5, 0.5) — non-zero, so a zero
    input row (MUL with the graph's empty row, an empty graph's pooled row) has A + b1 = b1 — and Wo [C][Dh] Xavier-uniform."""
    rng = np.random.default_rng(7000 + 131 * d_last + 17 * dh + c + 100003 * seed)
    l1, lo = np.sqrt(6.0 / (d_last + dh)), np.sqrt(6.0 / (c + dh))
    W1 = rng.uniform(-l1, l1, (dh, d_last)).astype(np.float32)
    b1 = rng.uniform(-0.5, 0.5, dh).astype(np.float32)
    Wo = rng.uniform(-lo, lo, (c, dh)).astype(np.float32)
    return W1, b1, Wo


def forward(cfg, g, kind, loss, sup, P2, W1, b1, Wo, act_name="relu", mask=None, graph_ptr=None, u=None, v=None, **kw):
    """fp64 step with the hidden layer.  g: the graph dict of tests/feature_cases.py; kind: one of KINDS (readout: mean over graph_ptr;
    pairs: u, v); loss / sup / mask as in pair_ref.forward, over the head's rows, the softmax's row maximum attached (head_model.loss
    says why); P2 = (W, a); W1 [Dh][D_last], b1 [Dh], Wo [C][Dh]; **kw: step_ref.forward's keywords.  -> the model's dict with Wo, W1,
    b1 (leaves), xin (grad retained), A and pre (numpy), z1 (grad retained), loss, y, loss_per_row."""
    head = HD.head(kind, loss, sup, mask, graph_ptr=graph_ptr, u=u, v=v, Wo=Wo, W1=W1, b1=b1, act_name=act_name, detach_max=False,
                   smooth_bce=True)
    return SR.forward(cfg, g["row_ptr"], g["col_idx"], None, g["x"], P2[0], P2[1], None, head=head, **kw)


def nonzero_min(a):
    a = np.abs(np.asarray(a))
    a = a[a != 0]
    return float(a.min()) if a.size else np.inf


def head_clear(out, loss, sup, mask):
    """The stage's own conditions on a model's outputs: every |A + b1| clear of the kink (zero rows of Xin included: there it is
    |b1|), and for softmax no trained row at the loss clamp."""
    if not float(np.abs(out["pre"]).min()) > A_MIN:
        return False
    if loss != SOFTMAX:
        return True
    keep = np.ones(len(out["y"]), bool) if mask is None else np.asarray(mask, bool)
    return float(out["y"][np.arange(len(out["y"])), np.asarray(sup)][keep].min()) > Y_MIN


# -- the cases of tests/test_head_mlp.py, shared with its CPU twin (the seed condition)
def families(FC):
    return list(FC.FAMILIES) + [D5_FAMILY]


def family(FC, name):
    return next(f for f in families(FC) if f[0] == name)


WIDTHS = (16, 5, 24)              # the head's register-blocked form, the scalar path of the row kernels, a padded softmax tile


def cases():
    """(family, variant, kind, loss, Dh, activation)"""
    out = [(f, "plain", k, SOFTMAX, dh, "relu") for f in ("records_d8", "generic", D5_FAMILY[0]) for k in KINDS for dh in WIDTHS]
    out += [("records_d8", "plain", k, SOFTMAX, 16, "lrelu") for k in KINDS]
    out += [("records_d8", "plain", k, BCE, 80, "relu") for k in ("pair_mul", "pair_add", "node")]            # C = 1
    out += [("records_d8", "plain", k, MSE, 16, "relu") for k in ("pair_mul", "readout", "node")]            # NaN holes
    out += [("records_d8", v, k, SOFTMAX, 16, "relu") for v in ("res_norm_reg", "fe3", "mask") for k in ("pair_mul", "node")]
    out += [(v, "plain", k, SOFTMAX, 16, "relu") for v in ("keep_taps", "bf16") for k in ("pair_mul", "node")]
    return out


def case_id(case):
    return "-".join(str(c) for c in case)


@functools.lru_cache(maxsize=None)
def _case_inputs(fam, variant, kind, loss, dh, act_name, n_rand=None):
    import __graft_entry__ as entry
    import feature_cases as FC
    pkg, orc = entry.load_package(), entry.load_oracle()
    g = FC.parity_graph()
    if loss == BCE:                                  # C = 1: the link-prediction head
        g = dict(g, c=1, labels=np.zeros(g["n"], np.int32))
    _, heads, outdims, kw = family(FC, fam)
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    bf16 = kw.get("dtype") == "bf16"
    graph_ptr = GRAPH_PTR if kind == "readout" else None
    u, v = (PR.pair_list(g["n"]) if n_rand is None else PR.pair_list(g["n"], n_rand=n_rand)) if kind.startswith("pair") else (None, None)
    R = len(u) if u is not None else len(graph_ptr) - 1 if graph_ptr is not None else g["n"]
    if loss == SOFTMAX:
        sup = g["labels"] if kind == "node" else PR.pair_labels(R, g["c"])
    elif loss == BCE:
        sup = (np.random.default_rng(41).random((R, 1)) > 0.5).astype(np.float32)
    else:
        sup = LR.targets_for(pkg, MSE, R, g["c"])    # NaN holes (loss_ref.MISSING)
    mask = LR.row_mask(R) if variant == "mask" else None
    W1, b1, Wo = head_values(outdims[-1], dh, g["c"])
    reg = FC.REG if variant == "res_norm_reg" else None
    keeps, attn, feat = FC.masks(cfg, g, cfg.heads, reg)
    model_kw = dict(eps=FC.EPS, keeps=keeps, attn=attn, feat=feat, bf16_pl=bf16)
    ea = EF.edge_attrs(g, FE) if variant == "fe3" else None

    def model(ps, P):
        inp = {}
        if variant == "fe3":
            inp = dict(ea=ea, We=SR.xavier_we(cfg, FE, ps))
        elif variant == "res_norm_reg":
            Wres, b = SR.xavier_wres(cfg, ps)
            gamma, beta = SR.ln_params(cfg, ps)
            inp = dict(Wres=Wres, b=b, gamma=gamma, beta=beta)
        return inp, forward(cfg, g, kind, loss, sup, P[:2], W1, b1, Wo, act_name, mask=mask, graph_ptr=graph_ptr, u=u, v=v, **inp, **model_kw)

    base = FC.CLEAR_V if variant == "res_norm_reg" else FC.CLEAR_HPRE
    P, inp, ref = FC.pick_params(orc, cfg, model, lambda r: base(r) and head_clear(r, loss, sup, mask))
    return dict(g=g, heads=heads, outdims=outdims, kw=kw, cfg=cfg, P=P[:2], inp=inp, seed=ref["seed"], kind=kind, loss=loss, sup=sup, mask=mask,
                dh=dh, act=act_name, W1=W1, b1=b1, Wo=Wo, graph_ptr=graph_ptr, u=u, v=v, rows=R, reg=reg, bf16=bf16, model_kw=model_kw)


def case_inputs(case, n_rand=None):
    """Everything a case runs on (cached: the seed search runs once per process).  A case without a clear seed among the 40 FAILS.
    n_rand: the random pairs of pair_ref.pair_list (None: its own count), for a longer pair list (tests/trip_cases.py)."""
    return dict(_case_inputs(*case) if n_rand is None else _case_inputs(*case, n_rand))


def model_of(ci, u=None, v=None):
    """The fp64 model of case_inputs' result (u, v: other pairs of the same length), after loss.backward()."""
    ref = forward(ci["cfg"], ci["g"], ci["kind"], ci["loss"], ci["sup"], ci["P"], ci["W1"], ci["b1"], ci["Wo"], ci["act"], mask=ci["mask"],
                  graph_ptr=ci["graph_ptr"], u=ci["u"] if u is None else u, v=ci["v"] if v is None else v, **ci["inp"], **ci["model_kw"])
    ref["loss"].backward()
    return ref


def make_ctx(pkg, ci, width=None, u=None, v=None, set_params=True, **kw):
    """A context of a case with the hidden layer (width: another width; 0: the call is made with width 0; False: not made), the parameter
    groups set and the gradients zeroed.  Without the layer Wo is a [C][D_last] slice of zeros + the case's values (the off tests compare
    two such contexts with each other).  **kw goes to GatContext on top of the family's keywords."""
    import feature_cases as FC
    A = pkg.abi
    g, inp, kind = ci["g"], ci["inp"], ci["kind"]
    ctx = pkg.GatContext(ci["heads"], ci["outdims"], g["f"], g["c"], **dict(ci["kw"], **kw))
    if inp.get("gamma") is not None:
        ctx.set_norm(eps=FC.EPS)
    if inp.get("We") is not None:
        ctx.set_edge_dim(FE)
    if inp.get("Wres") is not None or inp.get("b") is not None:
        ctx.set_residual(linear=inp.get("Wres") is not None, bias=inp.get("b") is not None)
    if ci["loss"] != SOFTMAX:
        ctx.set_loss(ci["loss"])
    width = ci["dh"] if width is None else width
    if width is not False:
        ctx.set_head_hidden(width, ci["act"])
    on = width not in (False, 0)
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    if kind == "readout":
        ctx.set_readout("mean", graph_ptr=ci["graph_ptr"])
    elif kind.startswith("pair"):
        ctx.set_pairs("mul" if kind == "pair_mul" else "add", ci["u"] if u is None else u, ci["v"] if v is None else v)
    if ci["loss"] == SOFTMAX:
        ctx.set_labels(ci["sup"])
    else:
        ctx.set_targets(ci["sup"])
    if inp.get("ea") is not None:
        ctx.set_edge_features(inp["ea"])
    if set_params:
        for grp, name in ((A.PARAM_WRES, "Wres"), (A.PARAM_B, "b"), (A.PARAM_LN_G, "gamma"), (A.PARAM_LN_B, "beta"), (A.PARAM_WE, "We")):
            if inp.get(name) is not None:
                ctx.params_set(grp, inp[name])
        ctx.params_set(A.PARAM_W, ci["P"][0]); ctx.params_set(A.PARAM_A, ci["P"][1])
        if on:
            assert width == ci["dh"]
            ctx.params_set(A.PARAM_WO, ci["Wo"]); ctx.params_set(A.PARAM_HEAD_W, ci["W1"]); ctx.params_set(A.PARAM_HEAD_B, ci["b1"])
        else:
            ctx.params_set(A.PARAM_WO, head_values(ci["outdims"][-1], ci["outdims"][-1], g["c"])[2])
    if ci["reg"] is not None:
        ctx.set_dropout(ci["reg"]["pf"], ci["reg"]["pa"], seed=ci["reg"]["seed"], first_step=0)
        ctx.set_dropedge(ci["reg"]["pe"])
    if ci["mask"] is not None:
        ctx.set_train_mask(ci["mask"])
    ctx.zero_grad()
    return ctx


def loss_rows(ci):
    """What the loss is divided by: the head's rows (softmax), the contributing target entries (BCE / MSE)."""
    if ci["loss"] == SOFTMAX:
        return ci["rows"]
    return max(1, int(LR.contributes(ci["sup"], ci["mask"]).sum()))
