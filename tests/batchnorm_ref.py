"""The fp64 autograd model of a training step WITH batch normalisation (include/gatv2_abi.h "batch normalisation"): the layer loop of
tests/step_ref.py (with the edge term of tests/edge_feat_ref.py) where a normalised layer takes its statistics down the COLUMNS of
u = h_pre [N][H*D] — over all N rows, whatever trains —
    training:  mu = mean_n u,  var = mean_n (u - mu)^2 (biased, two passes),  v = gamma * (u - mu) / sqrt(var + eps) + beta
               running_mean <- (1 - m) running_mean + m mu,   running_var <- (1 - m) running_var + m var N / (N - 1)   (N == 1: var)
    eval:      v = gamma * (u - running_mean) / sqrt(running_var + eps) + beta      (constants: nothing flows into them, nothing advances)
and hout = LReLU(v).  With bn=False it is step_ref.forward / edge_feat_ref.forward value for value (tests/test_batchnorm_cpu.py).  The
head is the node softmax + cross-entropy of step_ref, or — head=(kind, loss, sup, ...) — one of tests/head_mlp_ref.py's kinds."""
import numpy as np

import edge_feat_ref as EF
from step_ref import _nonzero_min, ln_offsets, res_offsets

MOMENTUM = 0.1


def stats_init(cfg):
    """(running_mean, running_var) of a fresh context: 0 and 1, flat [l][H_l*D_l]."""
    n = ln_offsets(cfg)[-1]
    return np.zeros(n), np.ones(n)


def running_update(run_mean, run_var, mu, var, n, momentum):
    """The running-statistics law on numpy arrays (var: the biased batch variance)."""
    unbiased = var * n / (n - 1) if n > 1 else var
    return (1 - momentum) * run_mean + momentum * mu, (1 - momentum) * run_var + momentum * unbiased


def welford_chan(u, chunks):
    """numpy restatement of the kernels' merge in fp64: per chunk of rows a Welford pass, the chunks folded in ascending order with Chan's
    formula.  u [N][C], chunks: list of row-index arrays (a partition of the rows).  -> (mean [C], biased var [C])."""
    n, m, q = 0.0, None, None
    for rows in chunks:
        if len(rows) == 0:
            continue
        nb, mb, qb = 0.0, np.zeros(u.shape[1]), np.zeros(u.shape[1])
        for r in rows:
            nb += 1.0
            d = u[r] - mb
            mb = mb + d / nb
            qb = qb + d * (u[r] - mb)
        if n == 0.0:
            n, m, q = nb, mb, qb
            continue
        tot = n + nb
        delta = mb - m
        m = m + delta * (nb / tot)
        q = q + qb + delta * delta * (n * (nb / tot))
        n = tot
    return m, q / n


def forward(cfg, row_ptr, col_idx, labels, X, W, a, Wo, ea=None, We=None, Wres=None, b=None, gamma=None, beta=None, eps=1e-5,
            skip_last=False, keeps=None, attn=None, feat=None, slope=0.01, bf16_pl=False, bn=True, training=True, running=None,
            momentum=MOMENTUM, head=None):
    """fp64 step.  Every argument of edge_feat_ref.forward with its meaning there; gamma / beta: the flat norm groups (None, both: no
    layer is normalised).  bn: the normalised layers are BATCH-normalised (False: layer-normalised, the model of step_ref).  training /
    running = (mean, var) flat [l][H_l*D_l] (None: 0 and 1) / momentum: see the module text.  head: None (node softmax + CE on labels
    with Wo [C][D_last]) or a callable  head(out) -> loss sum  on the model's dict (out["hout"][-1]: the last layer's rows).
    -> edge_feat_ref.forward's dict plus batch_mean / batch_rstd (flat numpy; training mode, normalised layers: else 0) and
    running_mean / running_var AFTER the step; v_min over every layer's v."""
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
        weo = EF.we_offsets(cfg, fe)
    run_mean, run_var = (np.asarray(r, np.float64).copy() for r in (stats_init(cfg) if running is None else running))
    bmean, brstd = np.zeros(lo[-1]), np.zeros(lo[-1])
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
        if bf16_pl:
            PL = PL + (PL.detach().to(torch.bfloat16).to(dt) - PL.detach())
        s = PL[src] + PR[dst]
        if ea is not None:
            s = s + torch.einsum("ef,hkf->ehk", eat[torch.from_numpy(np.flatnonzero(k)).long()], Wet[weo[l]:weo[l + 1]].view(H, D, fe))
        out["s_min"] = min(out["s_min"], _nonzero_min(s))
        e = (al * torch.nn.functional.leaky_relu(s, slope)).sum(-1)
        sc = np.zeros((H, E))
        sc[:, k] = e.detach().numpy().T
        out["score"].append(sc)
        m = torch.full((N, H), -1e9, dtype=dt).scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
        pe = torch.exp(e - m[dst])
        Z = torch.zeros((N, H), dtype=dt).index_add(0, dst, pe)
        alpha = pe / (Z[dst] + 1e-8)
        full = np.zeros((H, E))
        full[:, k] = (pe / Z[dst]).detach().numpy().T
        out["alpha"].append(full)
        w = alpha if attn is None else alpha * torch.from_numpy(np.asarray(attn[l], np.float64)[:, k].T)
        hpre = torch.zeros((N, H, D), dtype=dt).index_add(0, dst, w[..., None] * PL[src])
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
            sl = slice(lo[l], lo[l + 1])
            if not bn:                                       # step_ref's layer norm, operation for operation
                mu = u.mean(1, keepdim=True)
                var = ((u - mu) ** 2).mean(1, keepdim=True)
                v = (gt[sl] * (u - mu) / torch.sqrt(var + eps) + bet[sl]).view(N, H, D)
            elif training:
                mu = u.mean(0, keepdim=True)
                var = ((u - mu) ** 2).mean(0, keepdim=True)          # biased, two passes
                rstd = 1.0 / torch.sqrt(var + eps)
                bmean[sl] = mu.detach().numpy().ravel(); brstd[sl] = rstd.detach().numpy().ravel()
                run_mean[sl], run_var[sl] = running_update(run_mean[sl], run_var[sl], bmean[sl], var.detach().numpy().ravel(), N, momentum)
            else:
                mu = torch.from_numpy(run_mean[sl].copy()).view(1, -1)
                rstd = 1.0 / torch.sqrt(torch.from_numpy(run_var[sl].copy()).view(1, -1) + eps)
            if bn:
                v = (gt[sl] * ((u - mu) * rstd) + bet[sl]).view(N, H, D)
        out["v_min"] = min(out["v_min"], _nonzero_min(v))
        act = torch.nn.functional.leaky_relu(v, slope)
        x = act.mean(1) if last else act.reshape(N, H * D)
        if x.requires_grad:
            x.retain_grad()
        out["hpre"].append(hpre)
        out["hout"].append(x)
    out.update(batch_mean=bmean, batch_rstd=brstd, running_mean=run_mean, running_var=run_var)
    if head is not None:
        out["loss"] = head(out)
        return out
    z = x @ Wot.view(cfg.num_classes, cfg.outdims[-1]).t()
    ez = torch.exp(z - z.max(dim=1, keepdim=True).values.detach())
    y = ez / (ez.sum(1, keepdim=True) + 1e-8)
    lab = torch.from_numpy(np.asarray(labels)).long()
    out["loss"] = -torch.log(torch.clamp(y[torch.arange(N), lab], min=1e-12)).sum()
    return out


def head_of(kind, loss, sup, Wo, mask=None, graph_ptr=None, u=None, v=None, W1=None, b1=None, act_name="relu"):
    """forward's head= for one of tests/head_mlp_ref.py's kinds ("node", "readout": mean over graph_ptr, "pair_mul", "pair_add"), its
    loss modes (softmax / BCE / MSE on sup, over the head's rows, under mask) and, with W1 / b1, its hidden layer.  The leaves Wo (flat)
    and W1, b1 join the model's dict, with y."""
    import torch
    import head_mlp_ref as HM

    def head(out):
        leaf = lambda a_: torch.from_numpy(np.asarray(a_, np.float32).astype(np.float64).reshape(-1)).requires_grad_(True)
        xin = HM.head_input(out, kind, graph_ptr, u, v)
        Wot = leaf(Wo)
        out["Wo"] = Wot
        if W1 is not None:
            W1t, b1t = leaf(W1), leaf(b1)
            dh = b1t.shape[0]
            pre = xin @ W1t.view(dh, -1).t() + b1t
            xin = HM.act(pre, act_name)
            out.update(W1=W1t, b1=b1t, pre=pre.detach().numpy())
        z = xin @ Wot.view(-1, xin.shape[1]).t()
        total, y, _ = HM.head_loss(z, loss, sup, mask)
        out["y"] = y
        return total
    return head
