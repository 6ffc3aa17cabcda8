"""The fp64 autograd model of a training step with every feature of include/gatv2_abi.h the tests hold the kernels to: attention and
feature dropout ("dropout"), DropEdge per layer ("DropEdge"), the residual term and bias ("residual"),
    h_pre[n,h,d] += sum_f Wres_l[h*D+d][f] * x'_l[n][f] + b_l[h*D+d]          (x'_l: the layer's input after feature dropout)
and, in every normalised layer ("layer normalisation"),
    mu = mean_c u,  var = mean_c (u - mu)^2,  v = gamma * (u - mu) / sqrt(var + eps) + beta,  hout = LReLU(v)
over the H*D channels c of the row u = h_pre (residual term and bias included).  The score sees neither the residual nor the norm.
With every optional argument left out it is the model of tests/torch_ref.py, which stays the independent restatement it is pinned
against (tests/test_residual_cpu.py, tests/test_step_ref_cpu.py).  The mask hashes are in tests/dropout_ref.py and tests/dropedge_ref.py."""
import numpy as np


def _nonzero_min(t):
    """smallest |value| that is not exactly 0 (exact zeros — empty rows, dropped terms — take the same LeakyReLU' branch on
    both sides: max(x, slope*x) and x > 0)"""
    v = t.detach().abs()
    v = v[v > 0]
    return float(v.min()) if v.numel() else np.inf


def res_offsets(cfg):
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
    wo, bo = res_offsets(cfg)
    Wres = np.empty(wo[-1], np.float32)
    for l in range(cfg.L):
        hd = cfg.heads[l] * cfg.outdims[l]
        lim = np.sqrt(6.0 / (cfg.in_dims[l] + hd))
        Wres[wo[l]:wo[l + 1]] = rng.uniform(-lim, lim, wo[l + 1] - wo[l])
    b = rng.uniform(-0.5, 0.5, bo[-1]).astype(np.float32)
    return Wres, b


def ln_offsets(cfg):
    """ln_offsets [L+1] of the flat groups gamma and beta, [l][H_l*D_l] over all L layers."""
    o = [0]
    for l in range(cfg.L):
        o.append(o[-1] + cfg.heads[l] * cfg.outdims[l])
    return o


def ln_params(cfg, seed):
    """gamma ~ U[0.5, 1.5], beta ~ U[-0.5, 0.5] (test inputs: with gamma = 1, beta = 0 a wrong gamma factor would not show)."""
    rng = np.random.default_rng(2000 + seed)
    n = ln_offsets(cfg)[-1]
    return rng.uniform(0.5, 1.5, n).astype(np.float32), rng.uniform(-0.5, 0.5, n).astype(np.float32)


def forward(cfg, row_ptr, col_idx, labels, X, W, a, Wo, Wres=None, b=None, gamma=None, beta=None, eps=1e-5, skip_last=False,
            keeps=None, attn=None, feat=None, slope=0.01, bf16_pl=False, flat_lrelu_index=False):
    """fp64 step.  Wres / b: flat groups or None (that term absent).  gamma / beta: flat groups, or None (both): no layer is
    normalised.  skip_last: the last layer is left un-normalised.  keeps[l] [E] bool (DropEdge: every layer aggregates over its own
    reduced graph; None: all edges), attn[l] [H][E] on the full CSR, feat[l] [N][F_l] (None: no dropout of that kind).
    bf16_pl: the gathered table PL is used rounded to bf16 (nearest even) with a straight-through gradient — what bf16 storage
    computes; without it, bf16 rounding of PL moves scores across the LeakyReLU kink and the gradients differ by a few %.
    flat_lrelu_index: the output gradient takes LReLU'(h_pre) of the last layer at the reference's flat index n*D + d (E:598)
    instead of the exact [n,h,d]; ValueError with a normalised last layer, which gat_set_norm refuses too.
    -> dict(loss, hpre[l] (= u, grad retained: G = dL/dh_pre), hout[l] (grad retained: dL/dhout), alpha[l] (numpy [H][E]: the softmax
    over the surviving edges before the attention-dropout factor, pe / Z without the 1e-8 guard, 0 at dropped edges: GAT_TAP_ALPHA),
    s_min, hpre_min, v_min (smallest non-zero |s|, |h_pre|, |v| over the layers; v = h_pre in a layer left un-normalised), leaf
    tensors W, a, Wo, Wres, b, gamma, beta (None when absent))."""
    import torch
    dt = torch.float64
    assert (gamma is None) == (beta is None)
    if flat_lrelu_index and gamma is not None and not skip_last:
        raise ValueError("flat_lrelu_index with a normalised last layer")
    N = len(row_ptr) - 1
    E = int(row_ptr[-1])
    dst_all = np.repeat(np.arange(N), np.diff(row_ptr))
    leaf = lambda v: None if v is None else torch.tensor(np.asarray(v), dtype=dt, requires_grad=True)
    Wt, at, Wot, Wrt, bt, gt, bet = (leaf(v) for v in (W, a, Wo, Wres, b, gamma, beta))
    wro, bo = res_offsets(cfg)
    lo = ln_offsets(cfg)
    x = torch.tensor(np.asarray(X), dtype=dt)
    out = {"hpre": [], "hout": [], "alpha": [], "W": Wt, "a": at, "Wo": Wot, "Wres": Wrt, "b": bt, "gamma": gt, "beta": bet,
           "s_min": np.inf, "hpre_min": np.inf, "v_min": np.inf}
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
        if bf16_pl:                              # the gathered table rounded to bf16, straight-through gradient
            PL = PL + (PL.detach().to(torch.bfloat16).to(dt) - PL.detach())
        s = PL[src] + PR[dst]
        out["s_min"] = min(out["s_min"], _nonzero_min(s))
        e = (al * torch.nn.functional.leaky_relu(s, slope)).sum(-1)              # [E,H]
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
        out["hpre_min"] = min(out["hpre_min"], _nonzero_min(hpre))
        v = hpre
        if gt is not None and not (skip_last and last):
            u = hpre.reshape(N, H * D)
            mu = u.mean(1, keepdim=True)
            var = ((u - mu) ** 2).mean(1, keepdim=True)              # biased, two passes
            v = (gt[lo[l]:lo[l + 1]] * (u - mu) / torch.sqrt(var + eps) + bet[lo[l]:lo[l + 1]]).view(N, H, D)
        out["v_min"] = min(out["v_min"], _nonzero_min(v))
        if last and flat_lrelu_index:
            # value as always; the derivative factor of element [n,h,d] is LReLU' of the flat element n*D + d of h_pre (E:598)
            flat = hpre.detach().reshape(-1)[: N * D].view(N, 1, D).expand(N, H, D)      # v is h_pre here
            fac = torch.where(flat > 0, torch.ones((), dtype=dt), torch.full((), slope, dtype=dt))
            val = torch.nn.functional.leaky_relu(hpre.detach(), slope)
            act = val + (hpre - hpre.detach()) * fac
        else:
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
