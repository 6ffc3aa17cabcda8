"""Host restatement of the layer-normalisation contract of include/gatv2_abi.h ("layer normalisation"): the fp64 autograd model
of tests/residual_ref.py with, in every normalised layer,
    mu = mean_c u,  var = mean_c (u - mu)^2,  v = gamma * (u - mu) / sqrt(var + eps) + beta,  hout = LReLU(v)
over the H*D channels c of the row u = h_pre (residual term and bias included).  The score never sees the norm."""
import numpy as np

import dropout_ref as R
import residual_ref as RR


def offsets(cfg):
    """ln_offsets [L+1] of the flat groups gamma and beta, [l][H_l*D_l] over all L layers."""
    o = [0]
    for l in range(cfg.L):
        o.append(o[-1] + cfg.heads[l] * cfg.outdims[l])
    return o


def ln_params(cfg, seed):
    """gamma ~ U[0.5, 1.5], beta ~ U[-0.5, 0.5] (test inputs: with gamma = 1, beta = 0 a wrong gamma factor would not show)."""
    rng = np.random.default_rng(2000 + seed)
    n = offsets(cfg)[-1]
    return rng.uniform(0.5, 1.5, n).astype(np.float32), rng.uniform(-0.5, 0.5, n).astype(np.float32)


def forward(cfg, row_ptr, col_idx, labels, X, W, a, Wo, Wres=None, b=None, gamma=None, beta=None, eps=1e-5, skip_last=False,
            keeps=None, attn=None, feat=None, slope=0.01, bf16_pl=False):
    """fp64 step.  gamma / beta: flat groups, or None (both): no layer is normalised and the model is residual_ref.forward's.
    skip_last: the last layer is left un-normalised.  The other arguments as in residual_ref.forward.
    -> dict(loss, hpre[l] (= u, grad retained: G = dL/dh_pre), hout[l] (grad retained: dL/dhout), alpha[l] (numpy [H][E]: the softmax
    over the surviving edges before the attention-dropout factor, pe / Z without the 1e-8 guard, 0 at dropped edges: GAT_TAP_ALPHA), s_min, v_min (smallest non-zero |v| over the layers; |h_pre| of a
    layer left un-normalised), leaf tensors W, a, Wo, Wres, b, gamma, beta (None when absent))."""
    import torch
    dt = torch.float64
    assert (gamma is None) == (beta is None)
    N = len(row_ptr) - 1
    E = int(row_ptr[-1])
    dst_all = np.repeat(np.arange(N), np.diff(row_ptr))
    leaf = lambda v: None if v is None else torch.tensor(np.asarray(v), dtype=dt, requires_grad=True)
    Wt, at, Wot, Wrt, bt, gt, bet = (leaf(v) for v in (W, a, Wo, Wres, b, gamma, beta))
    wro, bo = RR.offsets(cfg)
    lo = offsets(cfg)
    x = torch.tensor(np.asarray(X), dtype=dt)
    out = {"hpre": [], "hout": [], "alpha": [], "W": Wt, "a": at, "Wo": Wot, "Wres": Wrt, "b": bt, "gamma": gt, "beta": bet,
           "s_min": np.inf, "v_min": np.inf}
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
        full = np.zeros((H, E))                                      # GAT_TAP_ALPHA: [H][E], exactly 0 at dropped edges
        full[:, k] = (pe / Z[dst]).detach().numpy().T                # the softmax itself: the model's weight above is within 1e-8 of it
        out["alpha"].append(full)
        w = alpha if attn is None else alpha * torch.from_numpy(np.asarray(attn[l], np.float64)[:, k].T)
        hpre = torch.zeros((N, H, D), dtype=dt).index_add(0, dst, w[..., None] * PL[src])
        if Wrt is not None:
            hpre = hpre + torch.einsum("nf,hkf->nhk", x, Wrt[wro[l]:wro[l + 1]].view(H, D, F))
        if bt is not None:
            hpre = hpre + bt[bo[l]:bo[l + 1]].view(1, H, D)
        if hpre.requires_grad:
            hpre.retain_grad()
        v = hpre
        if gt is not None and not (skip_last and l == cfg.L - 1):
            u = hpre.reshape(N, H * D)
            mu = u.mean(1, keepdim=True)
            var = ((u - mu) ** 2).mean(1, keepdim=True)              # biased, two passes
            v = (gt[lo[l]:lo[l + 1]] * (u - mu) / torch.sqrt(var + eps) + bet[lo[l]:lo[l + 1]]).view(N, H, D)
        out["v_min"] = min(out["v_min"], R._nonzero_min(v))
        act = torch.nn.functional.leaky_relu(v, slope)
        x = act.mean(1) if l == cfg.L - 1 else act.reshape(N, H * D)
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
