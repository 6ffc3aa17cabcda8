"""Host restatement of the residual / bias contract of include/gatv2_abi.h ("residual"): the fp64 autograd model of a step —
the per-layer model of tests/dropedge_ref.py (forward_layers) with
    h_pre[n,h,d] += sum_f Wres_l[h*D+d][f] * x'_l[n][f] + b_l[h*D+d]
where x'_l is the layer's input after feature dropout.  The score never sees the residual."""
import numpy as np

import dropout_ref as R


def offsets(cfg):
    """(wres_offsets [L+1], b_offsets [L+1]) of the flat groups [l][H_l*D_l][F_l] and [l][H_l*D_l]."""
    wo, bo = [0], [0]
    for l in range(cfg.L):
        hd = cfg.heads[l] * cfg.outdims[l]
        wo.append(wo[-1] + hd * cfg.in_dims[l])
        bo.append(bo[-1] + hd)
    return wo, bo


def xavier_wres(cfg, seed):
    """Some Xavier-uniform Wres (lim = sqrt(6 / (F + H*D)) per layer) and a non-zero b, from numpy's generator (test inputs;
    gat_params_init draws its own stream on the device)."""
    rng = np.random.default_rng(1000 + seed)
    wo, bo = offsets(cfg)
    Wres = np.empty(wo[-1], np.float32)
    for l in range(cfg.L):
        hd = cfg.heads[l] * cfg.outdims[l]
        lim = np.sqrt(6.0 / (cfg.in_dims[l] + hd))
        Wres[wo[l]:wo[l + 1]] = rng.uniform(-lim, lim, wo[l + 1] - wo[l])
    b = rng.uniform(-0.5, 0.5, bo[-1]).astype(np.float32)
    return Wres, b


def forward(cfg, row_ptr, col_idx, labels, X, W, a, Wo, Wres=None, b=None, keeps=None, attn=None, feat=None, slope=0.01,
            bf16_pl=False, flat_lrelu_index=False):
    """fp64 step.  Wres / b: flat groups or None (that term absent).  keeps[l] [E] bool (DropEdge, per layer), attn[l] [H][E],
    feat[l] [N][F_l] as in dropedge_ref.forward_layers.  flat_lrelu_index: the output gradient takes LReLU'(h_pre) of the last
    layer at the reference's flat index n*D + d (E:598) instead of the exact [n,h,d].
    -> dict(loss, hpre[l], s_min, hpre_min, W, a, Wo, Wres, b leaf tensors (Wres / b: None when absent))."""
    import torch
    dt = torch.float64
    N = len(row_ptr) - 1
    E = int(row_ptr[-1])
    dst_all = np.repeat(np.arange(N), np.diff(row_ptr))
    Wt = torch.tensor(np.asarray(W), dtype=dt, requires_grad=True)
    at = torch.tensor(np.asarray(a), dtype=dt, requires_grad=True)
    Wot = torch.tensor(np.asarray(Wo), dtype=dt, requires_grad=True)
    Wrt = None if Wres is None else torch.tensor(np.asarray(Wres), dtype=dt, requires_grad=True)
    bt = None if b is None else torch.tensor(np.asarray(b), dtype=dt, requires_grad=True)
    wro, bo = offsets(cfg)
    x = torch.tensor(np.asarray(X), dtype=dt)
    out = {"hpre": [], "W": Wt, "a": at, "Wo": Wot, "Wres": Wrt, "b": bt, "s_min": np.inf, "hpre_min": np.inf}
    for l in range(cfg.L):
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
        if bf16_pl:                              # the gathered table rounded to bf16, straight-through gradient
            PL = PL + (PL.detach().to(torch.bfloat16).to(dt) - PL.detach())
        s = PL[src] + PR[dst]
        out["s_min"] = min(out["s_min"], R._nonzero_min(s))
        e = (al * torch.nn.functional.leaky_relu(s, slope)).sum(-1)
        m = torch.full((N, H), -1e9, dtype=dt).scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
        pe = torch.exp(e - m[dst])
        Z = torch.zeros((N, H), dtype=dt).index_add(0, dst, pe)
        alpha = pe / (Z[dst] + 1e-8)
        w = alpha if attn is None else alpha * torch.from_numpy(np.asarray(attn[l], np.float64)[:, k].T)
        hpre = torch.zeros((N, H, D), dtype=dt).index_add(0, dst, w[..., None] * PL[src])
        if Wrt is not None:
            hpre = hpre + torch.einsum("nf,hkf->nhk", x, Wrt[wro[l]:wro[l + 1]].view(H, D, F))
        if bt is not None:
            hpre = hpre + bt[bo[l]:bo[l + 1]].view(1, H, D)
        out["hpre_min"] = min(out["hpre_min"], R._nonzero_min(hpre))
        if l == cfg.L - 1 and flat_lrelu_index:
            # value as always; the derivative factor of element [n,h,d] is LReLU' of the flat element n*D + d of h_pre (E:598)
            flat = hpre.detach().reshape(-1)[: N * D].view(N, 1, D).expand(N, H, D)
            fac = torch.where(flat > 0, torch.ones((), dtype=dt), torch.full((), slope, dtype=dt))
            val = torch.nn.functional.leaky_relu(hpre.detach(), slope)
            act = val + (hpre - hpre.detach()) * fac
        else:
            act = torch.nn.functional.leaky_relu(hpre, slope)
        x = act.mean(1) if l == cfg.L - 1 else act.reshape(N, H * D)
        out["hpre"].append(hpre)
    z = x @ Wot.view(cfg.num_classes, cfg.outdims[-1]).t()
    ez = torch.exp(z - z.max(dim=1, keepdim=True).values.detach())
    y = ez / (ez.sum(1, keepdim=True) + 1e-8)
    lab = torch.from_numpy(np.asarray(labels)).long()
    out["loss"] = -torch.log(torch.clamp(y[torch.arange(N), lab], min=1e-12)).sum()
    return out
