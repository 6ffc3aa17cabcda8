"""The references of the BCE / MSE output heads (include/gatv2_abi.h "loss modes of the output head"; TEST INFRASTRUCTURE).

1. The fp64 autograd model of a whole step: tests/step_ref.py::forward with the head of tests/head_model.py on the node rows or the
   pooled rows X, z = X Woᵀ and one of the two losses (max-form BCE), the NaN entries and the rows outside the mask removed from the sum.
2. A plain numpy fp64 reference of the head alone, in the style of tests/head_ref.py: y, l, dz, gH, gradWo from the head's own inputs,
   and `undecided`: the BCE entries whose |z| is below the fp32 rounding bound of that logit (their prediction z > 0 may come out
   either way in fp32) — except where the bound itself is 0: all products are exactly 0 there and z = 0 on any path.

    BCE  y = sigmoid(z)   l = max(z,0) - t z + log1p(exp(-|z|))   dz = y - t        correct: (z > 0) == (t > 0.5)
    MSE  y = z            l = (z - t)^2                           dz = 2 (z - t)    correct: never
Also what tests/test_loss_modes.py and tests/test_loss_modes_cpu.py share: the cases, the targets, the context builder."""
import functools
from typing import NamedTuple

import numpy as np

import head_model as HD
import readout_ref as RR
import step_ref as SR
from head_model import BCE, MSE, contributes
MODES = (BCE, MSE)
MISSING = 0.2


def forward(cfg, g, T, mode, P, mask=None, graph_ptr=None, readout=None, **kw):
    """fp64 step in loss mode `mode`.  g: the graph dict of tests/feature_cases.py (its labels are not used); T [rows][C] float with NaN
    = missing, mask [rows] or None — rows are nodes, or the graphs of graph_ptr when readout is "mean" / "sum" / "max"; **kw:
    step_ref.forward's keywords.  -> the model's dict with loss, y (numpy), z (numpy), X (the head's input rows)."""
    head = HD.head("node" if readout is None else "readout", mode, T, mask, graph_ptr=graph_ptr, pool_mode=readout)
    out = SR.forward(cfg, g["row_ptr"], g["col_idx"], None, g["x"], *P, head=head, **kw)
    out["X"] = out["xin"]
    return out


# -- the head alone
class LossHeadRef(NamedTuple):
    z: np.ndarray          # [R][C] float64
    y: np.ndarray          # [R][C]
    l: np.ndarray          # [R][C] per entry, 0 where the entry does not contribute
    dz: np.ndarray         # [R][C], 0 likewise
    gH: np.ndarray         # [R][D_last]
    gradWo: np.ndarray     # [C][D_last]
    on: np.ndarray         # [R][C] bool: contributes
    correct: np.ndarray    # [R][C] bool: contributes and (z > 0) == (t > 0.5) (BCE; all False for MSE)
    undecided: np.ndarray  # [R][C] bool: contributes and |z| below the entry's rounding bound (BCE; all False for MSE)
    bound: np.ndarray      # [R][C] the fp32 rounding bound of the logit


def logit_rounding_bound(X, Wo):
    """Per entry: (D_last + 1) 2⁻²⁴ Σ_j |Wo[c,j]| |X[r,j]| — D_last products and sums at unit round-off 2⁻²⁴ (the per-logit form of
    head_ref.logit_rounding_bound, which doubles it because the softmax loss is measured between two logits)."""
    X = np.abs(np.asarray(X, np.float64))
    DL = X.shape[1]
    aw = np.abs(np.asarray(Wo, np.float64).reshape(-1, DL))
    return (DL + 1) * 2.0 ** -24 * (X @ aw.T)


def head_ref(X, Wo, T, mask, mode) -> LossHeadRef:
    X = np.asarray(X, np.float64)
    DL = X.shape[1]
    Wo64 = np.asarray(Wo, np.float32).reshape(-1, DL).astype(np.float64)
    on = contributes(T, mask)
    t = np.where(on, np.nan_to_num(np.asarray(T, np.float64)), 0.0)
    z = X @ Wo64.T
    bound = logit_rounding_bound(X, Wo64)
    if mode == BCE:
        e = np.exp(-np.abs(z))
        y = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        l = np.maximum(z, 0.0) - t * z + np.log1p(e)
        dz = y - t
        correct = on & ((z > 0) == (t > 0.5))
        # bound == 0: every product Wo[c,j] X[r,j] is exactly 0 (a row without in-edges has X = 0), so z = 0 in any arithmetic: decided
        undecided = on & (np.abs(z) <= bound) & (bound > 0)
    else:
        y = z
        l = (z - t) ** 2
        dz = 2.0 * (z - t)
        correct = np.zeros_like(on)
        undecided = np.zeros_like(on)
    l = np.where(on, l, 0.0)
    dz = np.where(on, dz, 0.0)
    return LossHeadRef(z, y, l, dz, dz @ Wo64, dz.T @ X, on, correct, undecided, bound)


def count_bounds(ref):
    """(sure, slack): n_correct must lie in [sure, sure + slack]."""
    return int((ref.correct & ~ref.undecided).sum()), int(ref.undecided.sum())


# -- cases shared by the GPU tests and their CPU twin
def targets_for(pkg, mode, rows, C, seed=5, missing=MISSING):
    return pkg.synth.targets("multilabel" if mode == BCE else "regression", rows, C, seed=seed, missing=missing)


def row_mask(rows, seed=3):
    """~60 % of the rows train; the first and the last do not."""
    m = np.random.default_rng(seed).random(rows) > 0.4
    m[0] = m[-1] = False
    if rows > 2 and not m.any():
        m[1] = True
    return m


# whole-step cases on FC.parity_graph: (family name, variant, loss mode); every family plain, records_d8 also with the feature stack
# (residual + norm + the three regularisers) and with a training mask
STEP_VARIANTS = ("res_norm_reg", "mask")


def step_cases(FC):
    out = [(f[0], "plain", m) for f in FC.FAMILIES for m in MODES]
    out += [("records_d8", v, m) for v in STEP_VARIANTS for m in MODES]
    return out


# readout cases on RR.GRAPH_PTR: (pooling, variant, loss mode)
READOUT_CASES = [("mean", "plain", MSE), ("mean", "plain", BCE), ("max", "plain", MSE), ("max", "plain", BCE), ("mean", "fe3", MSE),
                 ("max", "mask", BCE)]


def case_id(case):
    return "-".join(str(c) for c in case)


@functools.lru_cache(maxsize=None)
def _step_inputs(family, variant, mode):
    import __graft_entry__ as entry
    import feature_cases as FC
    pkg, orc = entry.load_package(), entry.load_oracle()
    g = FC.parity_graph()
    _, heads, outdims, kw = next(f for f in FC.FAMILIES if f[0] == family)
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    bf16 = kw.get("dtype") == "bf16"
    if variant == "res_norm_reg":
        P, inp, ref = FC.pick_case(orc, cfg, g, FC.NORM_MODES[1], norm=True, reg=FC.REG, bf16_pl=bf16)
        reg = FC.REG
    else:
        P, inp, ref = FC.pick_case(orc, cfg, g, None, bf16_pl=bf16)
        inp, reg = {}, None
    keeps, attn, feat = FC.masks(cfg, g, cfg.heads, reg)
    T = targets_for(pkg, mode, g["n"], g["c"])
    mask = row_mask(g["n"]) if variant == "mask" else None
    return dict(g=g, heads=heads, outdims=outdims, kw=kw, cfg=cfg, P=P, inp=inp, seed=ref["seed"], T=T, mask=mask, reg=reg, bf16=bf16,
                mode=mode, graph_ptr=None, readout=None, model_kw=dict(eps=FC.EPS, keeps=keeps, attn=attn, feat=feat, bf16_pl=bf16))


def step_inputs(case):
    return dict(_step_inputs(*case))


@functools.lru_cache(maxsize=None)
def _readout_inputs(pool, variant, mode):
    import __graft_entry__ as entry
    import feature_cases as FC
    pkg, orc = entry.load_package(), entry.load_oracle()
    g, gp = FC.parity_graph(), RR.GRAPH_PTR
    heads, outdims, kw = [8, 8], [8, 8], {}
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    G = len(gp) - 1
    glab = RR.graph_labels(G, g["c"])           # (the seed search of readout_ref looks at the softmax clamp too: harmless here)
    gmask = RR.graph_mask(gp) if variant == "mask" else None
    P, inp, seed = RR.pick(FC, orc, cfg, g, gp, pool, glab, gmask, "fe3" if variant == "fe3" else "plain", False)
    T = targets_for(pkg, mode, G, g["c"], missing=MISSING)
    return dict(g=g, heads=heads, outdims=outdims, kw=kw, cfg=cfg, P=P, inp=inp, seed=seed, T=T, mask=gmask, reg=None, bf16=False, mode=mode,
                graph_ptr=gp, readout=pool, model_kw=dict(eps=FC.EPS, keeps=None, attn=None, feat=None, bf16_pl=False))


def readout_inputs(case):
    return dict(_readout_inputs(*case))


def model_of(ci):
    """The fp64 model of a case, after loss.backward()."""
    ref = forward(ci["cfg"], ci["g"], ci["T"], ci["mode"], ci["P"], mask=ci["mask"], graph_ptr=ci["graph_ptr"], readout=ci["readout"],
                  **ci["inp"], **ci["model_kw"])
    ref["loss"].backward()
    return ref


def make_ctx(pkg, ci, T=None, set_loss=True, **kw):
    """A context of a case in its loss mode, targets and mask set, the parameter groups set, the gradients zeroed.  **kw goes to
    GatContext on top of the family's keywords."""
    import feature_cases as FC
    A = pkg.abi
    g, inp = ci["g"], ci["inp"]
    ctx = pkg.GatContext(ci["heads"], ci["outdims"], g["f"], g["c"], **dict(ci["kw"], **kw))
    if inp.get("gamma") is not None:
        ctx.set_norm(eps=FC.EPS)
    if inp.get("We") is not None:
        ctx.set_edge_dim(RR.FE)
    if inp.get("Wres") is not None or inp.get("b") is not None:
        ctx.set_residual(linear=inp.get("Wres") is not None, bias=inp.get("b") is not None)
    if set_loss:
        ctx.set_loss(ci["mode"])
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    if ci["readout"] is not None:
        ctx.set_readout(ci["readout"], graph_ptr=ci["graph_ptr"])
    ctx.set_targets(ci["T"] if T is None else T)
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
    if ci["mask"] is not None:
        ctx.set_train_mask(ci["mask"])
    ctx.zero_grad()
    return ctx


# -- shards: two ranks on the host transport, BCE with missing entries, on FC.shard_problem
def shard_setup(pkg, orc):
    import feature_cases as FC
    g = FC.shard_problem()
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    return g, orc.xavier_params(cfg, 11), targets_for(pkg, BCE, g["n"], g["c"], seed=9)


def shard_worker(rank, world, outdir, shm):
    """One rank of a host-transport step in BCE mode: the shard's own target rows; loss, correct and the gradients to outdir/r<rank>.npz."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as entry
    pkg, orc = entry.load_package(), entry.load_oracle()
    g, P, T = shard_setup(pkg, orc)
    S = pkg.shard
    plan = S.make_plan(g["row_ptr"], world, rank)
    rp_l, ci_l = S.local_csr(plan, g["row_ptr"], g["col_idx"])
    lo, hi = plan.row0, plan.row0 + plan.n_rows
    ctx = pkg.GatContext([8, 8], [8, 8], g["f"], g["c"], device=0)
    ctx.set_loss(BCE)
    ctx.set_graph(rp_l, ci_l, n_table=plan.n_table, table_row0=plan.table_row0)
    ctx.set_features(g["x"][lo:hi])
    ctx.set_targets(S.local_targets(plan, T))
    for grp, arr in enumerate(P):
        ctx.params_set(grp, arr)
    ctx.comm_init_host(world, rank, shm, 4 * max(plan.n_table * 64, ctx.n_params + 3))
    ctx.zero_grad()
    loss, correct = ctx.step()
    grads = np.concatenate([ctx.grads_get(k) for k in range(3)])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), loss=loss, correct=correct, grads=grads)
    ctx.close()


def grads_min(ref):
    return RR.grads_min(ref)
