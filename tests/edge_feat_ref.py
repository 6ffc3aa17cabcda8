"""The fp64 autograd model of a training step WITH edge features (include/gatv2_abi.h "edge features"): tests/step_ref.py's forward
restated with two more arguments — the per-edge attributes ea [E][Fe] in CSR order and the flat parameter group We [l][H_l*D_l][Fe] —
and two more outputs, the leaf We and score[l] as [H][E] (GAT_TAP_SCORE).  The edge term sits inside the LeakyReLU of the score,
    s[j][c] = PL[src_j][c] + PR[dst][c] + sum_f We_l[c][f] * ea[j][f]
and nowhere else: the message stays PL[src].  s_min is taken over the new s.  With ea = None (or We = 0) it is step_ref.forward, value
for value (tests/test_edge_features_cpu.py pins that).

tests/step_ref.py is a yardstick of the earlier feature tests and is left as it is here; this module is to be folded into it by a
later change (two optional arguments there, and this file goes)."""
import numpy as np

from step_ref import _nonzero_min, ln_offsets, res_offsets


def we_offsets(cfg, fe):
    """we_offsets [L+1] of the flat group [l][H_l*D_l][Fe]."""
    o = [0]
    for l in range(cfg.L):
        o.append(o[-1] + cfg.heads[l] * cfg.outdims[l] * fe)
    return o


def xavier_we(cfg, fe, seed):
    """Some Xavier-uniform We (lim = sqrt(6 / (Fe + H*D)) per layer) from numpy's generator (test inputs; gat_params_init draws its
    own stream on the device)."""
    rng = np.random.default_rng(3000 + seed)
    o = we_offsets(cfg, fe)
    We = np.empty(o[-1], np.float32)
    for l in range(cfg.L):
        lim = np.sqrt(6.0 / (fe + cfg.heads[l] * cfg.outdims[l]))
        We[o[l]:o[l + 1]] = rng.uniform(-lim, lim, o[l + 1] - o[l])
    return We


def forward(cfg, row_ptr, col_idx, labels, X, W, a, Wo, ea=None, We=None, Wres=None, b=None, gamma=None, beta=None, eps=1e-5,
            skip_last=False, keeps=None, attn=None, feat=None, slope=0.01, bf16_pl=False):
    """fp64 step; every argument of step_ref.forward but flat_lrelu_index, with its meaning there.  ea [E][Fe] (rows of the FULL CSR;
    DropEdge takes the kept rows) and We flat [l][H_l*D_l][Fe]: both or neither.
    -> step_ref.forward's dict plus "We" (leaf, None without the feature) and "score" (per layer numpy [H][E]: the raw attention
    score sum_d a * LReLU(s), natural-log domain, 0 at dropped edges)."""
    import torch
    dt = torch.float64
    assert (gamma is None) == (beta is None) and (ea is None) == (We is None)
    N = len(row_ptr) - 1
    E = int(row_ptr[-1])
    dst_all = np.repeat(np.arange(N), np.diff(row_ptr))
    leaf = lambda v: None if v is None else torch.tensor(np.asarray(v), dtype=dt, requires_grad=True)
    Wt, at, Wot, Wrt, bt, gt, bet, Wet = (leaf(v) for v in (W, a, Wo, Wres, b, gamma, beta, We))
    wro, bo = res_offsets(cfg)
    lo = ln_offsets(cfg)
    if ea is not None:
        eat = torch.tensor(np.asarray(ea), dtype=dt)
        assert eat.shape[0] == E
        fe = eat.shape[1]
        weo = we_offsets(cfg, fe)
    x = torch.tensor(np.asarray(X), dtype=dt)
    out = {"hpre": [], "hout": [], "alpha": [], "score": [], "W": Wt, "a": at, "Wo": Wot, "Wres": Wrt, "b": bt, "gamma": gt, "beta": bet,
           "We": Wet, "s_min": np.inf, "hpre_min": np.inf, "v_min": np.inf}
    for l in range(cfg.L):
        last = l == cfg.L - 1
        k = np.ones(E, bool) if keeps is None else np.asarray(keeps[l], bool)
        dst = torch.from_numpy(dst_all[k]).long()
        src = torch.from_numpy(np.asarray(col_idx)[k]).long()
        H, D, F = cfg.heads[l], cfg.outdims[l], cfg.in_dims[l]
        if feat is not None:
            x = x * torch.from_numpy(np.asarray(feat[l], np.float64))
        Wl = Wt[cfg.w_offsets[l]:cfg.w_offsets[l + 1]].view(H, D, 2 * F)
        al = at[cfg.a_offsets[l]:cfg.a_offsets[l + 1]].view(H, D)
        PL = torch.einsum("nf,hkf->nhk", x, Wl[:, :, :F])
        PR = torch.einsum("nf,hkf->nhk", x, Wl[:, :, F:])
        if bf16_pl:                              # the gathered table rounded to bf16, straight-through gradient (PE stays fp32)
            PL = PL + (PL.detach().to(torch.bfloat16).to(dt) - PL.detach())
        s = PL[src] + PR[dst]
        if ea is not None:                       # the edge term: in the score only
            s = s + torch.einsum("ef,hkf->ehk", eat[torch.from_numpy(np.flatnonzero(k)).long()], Wet[weo[l]:weo[l + 1]].view(H, D, fe))
        out["s_min"] = min(out["s_min"], _nonzero_min(s))
        e = (al * torch.nn.functional.leaky_relu(s, slope)).sum(-1)              # [E,H]
        sc = np.zeros((H, E))
        sc[:, k] = e.detach().numpy().T
        out["score"].append(sc)
        m = torch.full((N, H), -1e9, dtype=dt).scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
        pe = torch.exp(e - m[dst])
        Z = torch.zeros((N, H), dtype=dt).index_add(0, dst, pe)
        alpha = pe / (Z[dst] + 1e-8)
        full = np.zeros((H, E))                                      # GAT_TAP_ALPHA: [H][E], exactly 0 at dropped edges
        full[:, k] = (pe / Z[dst]).detach().numpy().T
        out["alpha"].append(full)
        w = alpha if attn is None else alpha * torch.from_numpy(np.asarray(attn[l], np.float64)[:, k].T)
        hpre = torch.zeros((N, H, D), dtype=dt).index_add(0, dst, w[..., None] * PL[src])     # the message stays PL[src]
        if Wrt is not None:
            hpre = hpre + torch.einsum("nf,hkf->nhk", x, Wrt[wro[l]:wro[l + 1]].view(H, D, F))
        if bt is not None:
            hpre = hpre + bt[bo[l]:bo[l + 1]].view(1, H, D)
        if hpre.requires_grad:
            hpre.retain_grad()
        out["hpre_min"] = min(out["hpre_min"], _nonzero_min(hpre))
        v = hpre
        if gt is not None and not (skip_last and last):
            u = hpre.reshape(N, H * D)
            mu = u.mean(1, keepdim=True)
            var = ((u - mu) ** 2).mean(1, keepdim=True)              # biased, two passes
            v = (gt[lo[l]:lo[l + 1]] * (u - mu) / torch.sqrt(var + eps) + bet[lo[l]:lo[l + 1]]).view(N, H, D)
        out["v_min"] = min(out["v_min"], _nonzero_min(v))
        act = torch.nn.functional.leaky_relu(v, slope)
        x = act.mean(1) if last else act.reshape(N, H * D)
        if x.requires_grad:
            x.retain_grad()
        out["hpre"].append(hpre)
        out["hout"].append(x)
    z = x @ Wot.view(cfg.num_classes, cfg.outdims[-1]).t()
    ez = torch.exp(z - z.max(dim=1, keepdim=True).values.detach())
    y = ez / (ez.sum(1, keepdim=True) + 1e-8)
    lab = torch.from_numpy(np.asarray(labels)).long()
    out["loss"] = -torch.log(torch.clamp(y[torch.arange(N), lab], min=1e-12)).sum()
    return out


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
    import step_ref as SR
    ea = edge_attrs(g, fe)
    k, attn, feat = FC.masks(cfg, g, cfg.heads, reg)
    keeps = k if keeps is None else keeps

    def model(ps, P):
        inp = dict(ea=ea, We=xavier_we(cfg, fe, ps), Wres=None, b=None, gamma=None, beta=None)
        if res_norm:
            inp["Wres"], inp["b"] = SR.xavier_wres(cfg, ps)
            inp["gamma"], inp["beta"] = SR.ln_params(cfg, ps)
        return inp, forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, **inp, eps=FC.EPS, keeps=keeps, attn=attn,
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
    FC.compare(pkg, ctx, g, cfg, ref, loss, tol, TAPS, FC.GROUPS)
    check_we(pkg, ctx, ref, tol)


SHARD_FE = 3


def shard_inputs(orc, g):
    """(W, a, Wo, Wres, b), ea, We of the shard tests: both residual flags and the edge term."""
    import feature_cases as FC
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    return FC.shard_inputs(orc, g, norm=False), edge_attrs(g, SHARD_FE), xavier_we(cfg, SHARD_FE, 11)


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
