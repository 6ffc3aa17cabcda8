"""What tests/test_edge_features.py shares with its CPU twin and tests/pick_profiles.py (include/gatv2_abi.h "edge features"): the case
table, the attribute rows, the seed search against tests/step_ref.py::forward(ea=, We=), the context builder, the comparison and the
shard worker."""
import numpy as np

import step_ref as SR

# -- the cases of tests/test_edge_features.py, shared with its CPU twin (the seed condition)
FES = (1, 3, 8)                                  # list 1: every family x these x {plain, REG}
SHAPE_FE = 5                                     # list 2: every edge shape x both dtypes, norm + residual + REG


def edge_attrs(g, fe):
    """The attribute rows of a case: default_rng(77), standard normal, fp32, [E][fe]."""
    return np.random.default_rng(77).standard_normal((len(g["col_idx"]), fe)).astype(np.float32)


def pick(FC, orc, cfg, g, fe, reg, res_norm=False, bf16=False, keeps=None):
    """FC.pick_params for an edge-feature case: We of xavier_we(ps); with res_norm also Wres / b of xavier_wres(ps) and gamma / beta of
    ln_params(ps) (norm + both residual flags).  Bounds of the parent's tests: CLEAR_V with the norm, CLEAR_HPRE without.
    -> (W, a, Wo), dict(ea, We, Wres, b, gamma, beta), the model's outputs."""
    ea = edge_attrs(g, fe)
    k, attn, feat = FC.masks(cfg, g, cfg.heads, reg)
    keeps = k if keeps is None else keeps

    def model(ps, P):
        inp = dict(ea=ea, We=SR.xavier_we(cfg, fe, ps), Wres=None, b=None, gamma=None, beta=None)
        if res_norm:
            inp["Wres"], inp["b"] = SR.xavier_wres(cfg, ps)
            inp["gamma"], inp["beta"] = SR.ln_params(cfg, ps)
        return inp, SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, **inp, eps=FC.EPS, keeps=keeps, attn=attn,
                               feat=feat, bf16_pl=bf16)
    return FC.pick_params(orc, cfg, model, FC.CLEAR_V if res_norm else FC.CLEAR_HPRE)


# -- contexts and the shard worker of tests/test_edge_features.py
def make_ctx(pkg, g, heads, outdims, P, fe, ea=None, We=None, Wres=None, b=None, gamma=None, beta=None, reg=None, touch=True, **kw):
    """FC.make_ctx with the edge-feature calls in their places: set_edge_dim(fe) before the graph (touch=False: the call is not made),
    set_edge_features(ea) after it (ea None: not made), We into PARAM_WE.  Residual flags / the norm are switched on by the presence of
    Wres / b / gamma.  **kw goes to GatContext."""
    import feature_cases as FC
    ctx = pkg.GatContext(heads, outdims, g["f"], g["c"], **kw)
    if gamma is not None:
        ctx.set_norm(eps=FC.EPS)
    if touch:
        ctx.set_edge_dim(fe)                         # between the two: any order is allowed
    if Wres is not None or b is not None:
        ctx.set_residual(linear=Wres is not None, bias=b is not None)
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    ctx.set_labels(g["labels"])
    if ea is not None:
        ctx.set_edge_features(ea)
    for grp, arr in enumerate((*P, Wres, b, gamma, beta, We)):
        if arr is not None:
            ctx.params_set(grp, arr)
    if reg is not None:
        ctx.set_dropout(reg["pf"], reg["pa"], seed=reg["seed"], first_step=0)
        ctx.set_dropedge(reg["pe"])
    ctx.zero_grad()
    return ctx


# -- a context against the model (tests/test_edge_features.py, tests/pick_profiles.py)
TAPS = ["hpre", "hout", "G"]


def check_we(pkg, ctx, ref, tol):
    import parity
    want = ref["We"].grad.numpy()
    got = ctx.grads_get(pkg.abi.PARAM_WE)
    assert got.shape == want.shape and np.abs(want).max() > 0
    parity.check_rel("grad We", got, want, tol)


def compare_all(pkg, ctx, g, cfg, ref, loss, tol):
    """loss, the three taps of every layer and all eight gradient groups (a group the model does not have is empty on the device)."""
    import feature_cases as FC
    FC.compare(pkg, ctx, g, cfg, ref, loss, tol, TAPS, FC.GROUPS[:7])
    check_we(pkg, ctx, ref, tol)


SHARD_FE = 3


def shard_inputs(orc, g):
    """(W, a, Wo, Wres, b), ea, We of the shard tests: both residual flags and the edge term."""
    import feature_cases as FC
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    return FC.shard_inputs(orc, g, norm=False), edge_attrs(g, SHARD_FE), SR.xavier_we(cfg, SHARD_FE, 11)


def shard_worker(rank, world, outdir, shm):
    """One rank of a host-transport step on FC.shard_problem with both residual flags and edge features, the attribute rows cut by
    shard.local_edge_features: loss, correct and all the gradient groups go to outdir/r<rank>.npz."""
    import os
    import sys
    import feature_cases as FC
    sys.path.insert(0, FC.ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package(); orc = entry.load_oracle()
    A = pkg.abi
    g = FC.shard_problem()
    S = pkg.shard
    plan = S.make_plan(g["row_ptr"], world, rank)
    rp_l, ci_l = S.local_csr(plan, g["row_ptr"], g["col_idx"])
    lo, hi = plan.row0, plan.row0 + plan.n_rows
    inputs, ea, We = shard_inputs(orc, g)
    ctx = pkg.GatContext([8, 8], [8, 8], g["f"], g["c"], device=0)
    ctx.set_residual(linear=True, bias=True)
    ctx.set_edge_dim(SHARD_FE)
    ctx.set_graph(rp_l, ci_l, n_table=plan.n_table, table_row0=plan.table_row0)
    ctx.set_features(g["x"][lo:hi])
    ctx.set_labels(g["labels"][lo:hi])
    ctx.set_edge_features(S.local_edge_features(plan, g["row_ptr"], ea))
    for grp, arr in enumerate(inputs):
        ctx.params_set(grp, arr)
    ctx.params_set(A.PARAM_WE, We)
    ctx.comm_init_host(world, rank, shm, 4 * max(plan.n_table * 64, ctx.n_params + 3))
    ctx.zero_grad()
    loss, correct = ctx.step()
    grads = np.concatenate([ctx.grads_get(k) for k in A.PARAM_GROUPS])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), loss=loss, correct=correct, grads=grads)
    ctx.close()
