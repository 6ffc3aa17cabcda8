"""The fp64 autograd model of a training step with a graph-level readout (include/gatv2_abi.h "graph-level readout"):
tests/step_ref.py::forward with the readout head of tests/head_model.py — the last hout, still attached to the autograd graph, is
pooled per graph,
    sum:  P[g] = sum_n X[n]        mean: P[g] = (sum_n X[n]) / cnt_g        max: P[g][d] = max_n X[n][d], the FIRST row attaining it
(an empty graph: P[g] = 0, no gradient), and the softmax + cross-entropy runs on the G pooled rows with the graph labels.
Also what tests/test_readout.py and tests/test_readout_cpu.py share: the cases, the seed search, the context builder."""
import functools

import numpy as np

import edge_feat_ref as EF
import head_model as HD
import step_ref as SR

MODES = ("mean", "sum", "max")
# The model's loss clamps y[label] at 1e-12 (step_ref.forward, E:527), and autograd gives a clamped graph NO gradient; the kernels form
# dz = y - onehot whatever y is (E:571-573), as the reference does.  The two agree only where the clamp is inactive — a condition on
# the inputs like the kinks, reached easily by SUM (a pooled row is 100 times a node's row, the softmax saturates): a case needs
# y[label] > Y_MIN for every graph that trains, three decades above the clamp (fp32 rounding of y is far below that).
Y_MIN = 1e-9
# The model's softmax is pe / (Z + 1e-8) (E:381's guard).  Where every row that receives gradient has ONE in-edge — MAX over a single
# graph picks such rows: nothing averages them down — the true gradient of `a` is exactly 0, which the kernels give, and the model
# keeps only the guard's artefact, about 1e-9: a comparison relative to max-abs has no scale there.  A case needs every compared
# parameter gradient of the model above GRAD_MIN in max-abs, three decades over the artefact.
GRAD_MIN = 1e-6
GAP = 1e-4            # a MAX case needs (largest - second largest) > GAP * max|X| in every (graph, column): both sides pick the same row


def node_graph(graph_ptr):
    gp = np.asarray(graph_ptr, np.int64)
    return np.repeat(np.arange(len(gp) - 1), np.diff(gp))


def pool(X, graph_ptr, mode):
    """X [N][DL] torch fp64 -> (P [G][DL] (autograd through X), argmax [G][DL] int64 numpy, -1 outside MAX / for an empty graph)."""
    import torch
    gp = np.asarray(graph_ptr, np.int64)
    G, DL = len(gp) - 1, X.shape[1]
    arg = np.full((G, DL), -1, np.int64)
    if mode in ("sum", "mean"):
        P = torch.zeros((G, DL), dtype=X.dtype).index_add(0, torch.from_numpy(node_graph(gp)).long(), X)
        if mode == "mean":
            cnt = torch.from_numpy(np.maximum(np.diff(gp), 1).astype(np.float64))      # (an empty graph's sum is 0 already)
            P = P / cnt[:, None]
        return P, arg
    assert mode == "max"
    rows = []
    cols = torch.arange(DL)
    for g in range(G):
        b, e = int(gp[g]), int(gp[g + 1])
        if e == b:
            rows.append(torch.zeros(DL, dtype=X.dtype))
            continue
        idx = np.argmax(X[b:e].detach().numpy(), axis=0)                             # first occurrence
        arg[g] = b + idx
        rows.append(X[torch.from_numpy(b + idx).long(), cols])
    return torch.stack(rows), arg


def pool_gap(X, graph_ptr, mode):
    """Smallest gap over (g, d) between the largest and the second-largest X[n][d] of a graph with at least 2 rows; inf outside MAX."""
    if mode != "max":
        return np.inf
    x = np.asarray(X, np.float64)
    gp = np.asarray(graph_ptr, np.int64)
    gap = np.inf
    for g in range(len(gp) - 1):
        b, e = int(gp[g]), int(gp[g + 1])
        if e - b >= 2:
            top = np.sort(x[b:e], axis=0)
            gap = min(gap, float((top[-1] - top[-2]).min()))
    return gap


def forward(cfg, g, graph_ptr, mode, glabels, P, gmask=None, **kw):
    """fp64 step with readout.  g: the graph dict of tests/feature_cases.py (its node labels are not used), glabels [G], gmask [G] bool
    or None (graphs outside it: no loss), **kw: step_ref.forward's keywords.
    -> the model's dict with loss (over the graphs), y [G][C], pooled (grad retained), argmax, pool_gap, x_max = max|X|."""
    out = SR.forward(cfg, g["row_ptr"], g["col_idx"], None, g["x"], *P, **kw,
                     head=HD.head("readout", HD.SOFTMAX, glabels, gmask, graph_ptr=graph_ptr, pool_mode=mode))
    X = out["hout"][-1].detach()
    G = len(graph_ptr) - 1
    keep = np.ones(G, bool) if gmask is None else np.asarray(gmask, bool)
    out["pooled"], out["loss_per_graph"], out["argmax"] = out["xin"], out["loss_per_row"], pool(X, graph_ptr, mode)[1]
    out["y_label_min"] = float(out["y"][np.arange(G), np.asarray(glabels)][keep].min())
    out["pool_gap"] = pool_gap(X.numpy(), graph_ptr, mode)
    out["x_max"] = float(X.abs().max())
    return out


# -- the cases of tests/test_readout.py, shared with its CPU twin (the seed condition)
GRAPH_PTR = [0, 0, 1, 40, 41, 150]               # on FC.parity_graph: an empty graph, two single-node graphs, 39 and 109 nodes
D5_FAMILY = ("d5_scalar", [4, 2], [8, 5], {})    # D_last = 5: the scalar-load path of the pooling
VARIANTS = ("res_norm_reg", "fe3", "mask")       # for records_d8 and generic, beside the plain case of every family
FE = 3


def families(FC):
    return list(FC.FAMILIES) + [D5_FAMILY]


def cases(FC):
    """(family name, heads, outdims, GatContext keywords, variant, mode)"""
    out = [(n, h, d, kw, "plain", m) for n, h, d, kw in families(FC) for m in MODES]
    out += [(n, h, d, kw, v, m) for n, h, d, kw in FC.FAMILIES if n in ("records_d8", "generic") for v in VARIANTS for m in MODES]
    return out


def case_id(case):
    return f"{case[0]}-{case[4]}-{case[5]}"


# a step that crosses a segment boundary of the pooling: (graph_ptr, mode, e) on FC.make_graph(5, n=600, e=e), family records_d8.
# BOUNDARY: the graph with 2500 + 300 edges.  2800 edges x 64 channels x 2 layers leave a score within 1e-5 of the LeakyReLU kink under
# about 999 Xavier seeds of 1000 (what FC.parity_graph's docstring says of 4000 edges; none of the first 40 is clear: largest s_min
# 7.7e-6), so these cases search BOUNDARY_SEEDS behind the first 40: seeds found with this module's own predicate by a scan of
# orc.xavier_params(cfg, 0 .. 35000), listed so that a test checks a handful of models instead of thousands.  The predicate is applied
# to whatever seed is taken: a listed seed that is not clear is passed over, and a case without a clear seed fails.
# BOUNDARY_SPARSE runs the same rows and graph_ptr on the graph with 1200 + 300 edges, where one of the first 40 seeds is clear.
# (G = 1 with MAX is not among the sparse ones: the 8 rows that win the maximum have a single in-edge each there, see GRAD_MIN.)
BOUNDARY = [(gp, m, 2500) for gp in ([0, 300, 600], [0, 600]) for m in ("mean", "max")]
BOUNDARY_SPARSE = [([0, 300, 600], "mean", 1200), ([0, 300, 600], "max", 1200), ([0, 600], "mean", 1200)]


def boundary_id(b):
    return f"G{len(b[0]) - 1}-{b[1]}-e{b[2]}"


def graph_labels(n_graphs, c, seed=31):
    return np.random.default_rng(seed).integers(0, c, n_graphs).astype(np.int32)


def label_prob_min(X, Wo, graph_ptr, mode, glabels, gmask=None):
    """Smallest y[g][label_g] over the graphs that train, of the head on the pooled rows of X (torch fp64, numpy Wo [C][DL])."""
    P = pool(X.detach(), graph_ptr, mode)[0].numpy()
    z = P @ np.asarray(Wo, np.float64).T
    ez = np.exp(z - z.max(1, keepdims=True))
    y = ez / (ez.sum(1, keepdims=True) + 1e-8)
    keep = np.ones(len(P), bool) if gmask is None else np.asarray(gmask, bool)
    return float(y[np.arange(len(P)), np.asarray(glabels)][keep].min())


def with_gap(base, graph_ptr, mode, glabels, gmask=None):
    """The feature's kink predicate `base` plus the readout's two conditions, on the node model's outputs (hout of the last layer, Wo):
    a clear winner for MAX, and no trained graph at the loss clamp (Y_MIN)."""
    def clear(ref):
        if not base(ref):
            return False
        X = ref["hout"][-1]
        Wo = ref["Wo"].detach().numpy().reshape(-1, X.shape[1])
        if label_prob_min(X, Wo, graph_ptr, mode, glabels, gmask) <= Y_MIN:
            return False
        x = X.detach().numpy()
        return pool_gap(x, graph_ptr, mode) > GAP * np.abs(x).max()
    return clear


BOUNDARY_SEEDS = (584, 5897)


def grads_min(ref):
    """Smallest max-abs over the model's parameter gradients (after loss.backward())."""
    return min(float(ref[k].grad.abs().max()) for k in SR.GROUPS[:8] if ref.get(k) is not None)


def pick_boundary(FC, orc, cfg, g, graph_ptr, mode, glabels):
    """pick() of a BOUNDARY case: the first 40 seeds, then BOUNDARY_SEEDS, under the same predicate plus GRAD_MIN on the readout model."""
    clear = with_gap(FC.CLEAR_HPRE, graph_ptr, mode, glabels)
    for ps in (*range(40), *BOUNDARY_SEEDS):
        P = orc.xavier_params(cfg, ps)
        if not clear(FC.run_model(cfg, g, P)):
            continue
        ref = forward(cfg, g, graph_ptr, mode, glabels, P)
        ref["loss"].backward()
        if grads_min(ref) > GRAD_MIN:
            return P, {}, ps
    raise AssertionError("no parameter seed clear of the LeakyReLU kink, the MAX ties, the loss clamp and the softmax guard")


def pick(FC, orc, cfg, g, graph_ptr, mode, glabels, gmask=None, variant="plain", bf16=False):
    """The parameter seed of a case: the first of 40 whose node model is clear of the LeakyReLU kinks at the bounds of the feature's own
    tests AND, for MAX, has a clear winner in every (graph, column), AND keeps every trained graph off the loss clamp.  The kink and MAX
    conditions do not depend on the labels, so the search runs on the node model (FC.pick_case; edge features: FC.pick_params on
    step_ref.forward).  -> (W, a, Wo), dict of the other inputs, seed."""
    if variant == "fe3":
        ea = EF.edge_attrs(g, FE)

        def model(ps, P):
            inp = dict(ea=ea, We=SR.xavier_we(cfg, FE, ps))
            return inp, SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, **inp, bf16_pl=bf16)
        P, inp, ref = FC.pick_params(orc, cfg, model, with_gap(FC.CLEAR_HPRE, graph_ptr, mode, glabels, gmask))
        return P, inp, ref["seed"]
    if variant == "res_norm_reg":
        P, inp, ref = FC.pick_case(orc, cfg, g, FC.NORM_MODES[1], norm=True, reg=FC.REG, bf16_pl=bf16,
                                   clear=with_gap(FC.CLEAR_V, graph_ptr, mode, glabels, gmask))
        return P, inp, ref["seed"]
    P, inp, ref = FC.pick_case(orc, cfg, g, None, bf16_pl=bf16, clear=with_gap(FC.CLEAR_HPRE, graph_ptr, mode, glabels, gmask))
    return P, {}, ref["seed"]


def graph_mask(graph_ptr):
    """The per-graph training mask of the "mask" variant: every graph but the last non-empty one."""
    cnt = np.diff(np.asarray(graph_ptr))
    m = np.ones(len(cnt), bool)
    m[np.flatnonzero(cnt > 0)[-1]] = False
    return m


@functools.lru_cache(maxsize=None)
def _case_inputs(family, variant, mode, boundary):
    import __graft_entry__ as entry
    import feature_cases as FC
    orc = entry.load_oracle()
    if boundary is None:
        g, gp = FC.parity_graph(), GRAPH_PTR
        _, heads, outdims, kw = next(f for f in families(FC) if f[0] == family)
    else:
        g, gp = FC.make_graph(5, n=600, e=boundary[1]), list(boundary[0])
        heads, outdims, kw = [8, 8], [8, 8], {}
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    bf16 = kw.get("dtype") == "bf16"
    glab = graph_labels(len(gp) - 1, g["c"])
    gmask = graph_mask(gp) if variant == "mask" else None
    if boundary is not None and boundary[1] == 2500:
        P, inp, seed = pick_boundary(FC, orc, cfg, g, gp, mode, glab)
    else:
        P, inp, seed = pick(FC, orc, cfg, g, gp, mode, glab, gmask, variant, bf16)
    reg = FC.REG if variant == "res_norm_reg" else None
    keeps, attn, feat = FC.masks(cfg, g, cfg.heads, reg)
    return dict(g=g, graph_ptr=gp, heads=heads, outdims=outdims, kw=kw, cfg=cfg, P=P, inp=inp, seed=seed, glabels=glab, gmask=gmask,
                reg=reg, bf16=bf16, model_kw=dict(eps=FC.EPS, keeps=keeps, attn=attn, feat=feat, bf16_pl=bf16))


def case_inputs(case=None, boundary=None):
    """Everything a case runs on (cached: the seed search runs once per process).  case: an entry of cases(); boundary: an entry of
    BOUNDARY / BOUNDARY_SPARSE (family records_d8, plain)."""
    if boundary is not None:
        return dict(_case_inputs("records_d8", "plain", boundary[1], (tuple(boundary[0]), boundary[2])), mode=boundary[1])
    return dict(_case_inputs(case[0], case[4], case[5], None), mode=case[5])


def model_of(ci):
    """The fp64 model of case_inputs' result, after loss.backward()."""
    ref = forward(ci["cfg"], ci["g"], ci["graph_ptr"], ci["mode"], ci["glabels"], ci["P"], gmask=ci["gmask"], **ci["inp"], **ci["model_kw"])
    ref["loss"].backward()
    return ref


def make_ctx(pkg, ci, mode=None, **kw):
    """A context of a case with readout `mode` (default: the case's; 0 / "none": the call is made with mode 0; False: not made), the
    parameter groups set and the gradients zeroed.  **kw goes to GatContext on top of the family's keywords."""
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
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    mode = ci["mode"] if mode is None else mode
    if mode is not False:
        ctx.set_readout(mode, graph_ptr=ci["graph_ptr"])
    readout = mode not in (False, 0, "none")
    ctx.set_labels(ci["glabels"] if readout else g["labels"])
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
    if readout and ci["gmask"] is not None:
        ctx.set_train_mask(ci["gmask"])
    ctx.zero_grad()
    return ctx
