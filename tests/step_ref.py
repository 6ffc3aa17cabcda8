"""The fp64 autograd model of a training step with every feature of include/gatv2_abi.h the tests hold the kernels to: attention and
feature dropout ("dropout"), DropEdge per layer ("DropEdge"), the residual term and bias ("residual"),
    h_pre[n,h,d] += sum_f Wres_l[h*D+d][f] * x'_l[n][f] + b_l[h*D+d]          (x'_l: the layer's input after feature dropout)
the edge term inside the LeakyReLU of the score and nowhere else ("edge features": the message stays PL[src]),
    s[j][c] = PL[src_j][c] + PR[dst][c] + sum_f We_l[c][f] * ea[j][f]
and, in every normalised layer, over the H*D channels c of the row u = h_pre (residual term and bias included), either
    mu = mean_c u,  var = mean_c (u - mu)^2,  v = gamma * (u - mu) / sqrt(var + eps) + beta,  hout = LReLU(v)     ("layer normalisation")
or ("batch normalisation") the same with the statistics taken down the COLUMNS of u [N][H*D] — over all N rows, whatever trains:
    training:  mu = mean_n u,  var = mean_n (u - mu)^2 (biased, two passes),  v = gamma * (u - mu) / sqrt(var + eps) + beta
               running_mean <- (1 - m) running_mean + m mu,   running_var <- (1 - m) running_var + m var N / (N - 1)   (N == 1: var)
    eval:      v = gamma * (u - running_mean) / sqrt(running_var + eps) + beta      (constants: nothing flows into them, nothing advances)
The score sees neither the residual nor the norm.  The head behind the last layer is the node softmax + cross-entropy, or any head of
tests/head_model.py.  With every optional argument left out it is the model of tests/torch_ref.py, which stays the independent
restatement it is pinned against (tests/test_residual_cpu.py, tests/test_step_ref_cpu.py).  The mask hashes are in
tests/dropout_ref.py and tests/dropedge_ref.py."""
import numpy as np

import head_model

GROUPS = "W a Wo Wres b gamma beta We W1 b1".split()          # GAT_PARAM_W .. GAT_PARAM_HEAD_B, in the ABI's order


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
            keeps=None, attn=None, feat=None, slope=0.01, bf16_pl=False, flat_lrelu_index=False, ea=None, We=None, bn=False,
            training=True, running=None, momentum=0.1, head=None):
    """fp64 step.  Wres / b: flat groups or None (that term absent).  gamma / beta: flat groups, or None (both): no layer is
    normalised.  skip_last: the last layer is left un-normalised.  keeps[l] [E] bool (DropEdge: every layer aggregates over its own
    reduced graph; None: all edges), attn[l] [H][E] on the full CSR, feat[l] [N][F_l] (None: no dropout of that kind).
    bf16_pl: the gathered table PL is used rounded to bf16 (nearest even) with a straight-through gradient — what bf16 storage
    computes; without it, bf16 rounding of PL moves scores across the LeakyReLU kink and the gradients differ by a few %.
    flat_lrelu_index: the output gradient takes LReLU'(h_pre) of the last layer at the reference's flat index n*D + d (E:598)
    instead of the exact [n,h,d]; ValueError with a normalised last layer — layer or batch norm — which gat_set_norm and
    gat_set_batch_norm refuse too.
    ea [E][Fe] (rows of the FULL CSR; DropEdge takes the kept rows) and We flat [l][H_l*D_l][Fe]: the edge term, both or neither.
    bn: the normalised layers are BATCH-normalised; training / running = (mean, var) flat [l][H_l*D_l] (None: 0 and 1) / momentum: see
    the module text.
    head: a callable head(out) -> loss sum on this dict once the layers are done, out["hout"][-1] still attached (tests/head_model.py::
    head; labels and Wo may then be None).  None: the node softmax + cross-entropy on labels with Wo [C][D_last].
    -> dict(loss, hpre[l] (= u, grad retained: G = dL/dh_pre), hout[l] (grad retained: dL/dhout), alpha[l] (numpy [H][E]: the softmax
    over the surviving edges before the attention-dropout factor, pe / Z without the 1e-8 guard, 0 at dropped edges: GAT_TAP_ALPHA),
    score[l] (numpy [H][E]: the raw attention score sum_d a * LReLU(s), natural-log domain, 0 at dropped edges: GAT_TAP_SCORE),
    s_min, hpre_min, v_min (smallest non-zero |s|, |h_pre|, |v| over the layers; v = h_pre in a layer left un-normalised), leaf
    tensors W, a, Wo, Wres, b, gamma, beta, We (None when absent), what the head adds and, with bn, batch_mean / batch_rstd (flat numpy;
    training mode, normalised layers: else 0) and running_mean / running_var AFTER the step)."""
    import torch
    dt = torch.float64
    assert (gamma is None) == (beta is None) and (ea is None) == (We is None)
    if flat_lrelu_index and gamma is not None and not skip_last:
        raise ValueError("flat_lrelu_index with a normalised last layer")
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
    if bn:
        import batchnorm_ref as BR
        run_mean, run_var = (np.asarray(r, np.float64).copy() for r in (BR.stats_init(cfg) if running is None else running))
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
        if bf16_pl:                              # the gathered table rounded to bf16, straight-through gradient (PE stays fp32)
            PL = PL + (PL.detach().to(torch.bfloat16).to(dt) - PL.detach())
        s = PL[src] + PR[dst]
        if ea is not None:                       # the edge term: in the score only
            s = s + torch.einsum("ef,hkf->ehk", eat[torch.from_numpy(np.flatnonzero(k)).long()], Wet[weo[l]:weo[l + 1]].view(H, D, fe))
        out["s_min"] = min(out["s_min"], _nonzero_min(s))
        e = (al * torch.nn.functional.leaky_relu(s, slope)).sum(-1)              # [E,H]
        sc = np.zeros((H, E))                                        # GAT_TAP_SCORE: [H][E], 0 at dropped edges
        sc[:, k] = e.detach().numpy().T
        out["score"].append(sc)
        m = torch.full((N, H), -1e9, dtype=dt).scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
        pe = torch.exp(e - m[dst])
        Z = torch.zeros((N, H), dtype=dt).index_add(0, dst, pe)
        alpha = pe / (Z[dst] + 1e-8)
        full = np.zeros((H, E))                                      # GAT_TAP_ALPHA: [H][E], exactly 0 at dropped edges
        full[:, k] = (pe / Z[dst]).detach().numpy().T                # the softmax itself: the model's weight above is within 1e-8 of it
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
            sl = slice(lo[l], lo[l + 1])
            if not bn:
                mu = u.mean(1, keepdim=True)
                var = ((u - mu) ** 2).mean(1, keepdim=True)              # biased, two passes
                v = (gt[sl] * (u - mu) / torch.sqrt(var + eps) + bet[sl]).view(N, H, D)
            else:
                if training:
                    mu = u.mean(0, keepdim=True)
                    var = ((u - mu) ** 2).mean(0, keepdim=True)          # biased, two passes
                    rstd = 1.0 / torch.sqrt(var + eps)
                    bmean[sl] = mu.detach().numpy().ravel(); brstd[sl] = rstd.detach().numpy().ravel()
                    run_mean[sl], run_var[sl] = BR.running_update(run_mean[sl], run_var[sl], bmean[sl], var.detach().numpy().ravel(), N,
                                                                  momentum)
                else:
                    mu = torch.from_numpy(run_mean[sl].copy()).view(1, -1)
                    rstd = 1.0 / torch.sqrt(torch.from_numpy(run_var[sl].copy()).view(1, -1) + eps)
                v = (gt[sl] * ((u - mu) * rstd) + bet[sl]).view(N, H, D)
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
    if bn:
        out.update(batch_mean=bmean, batch_rstd=brstd, running_mean=run_mean, running_var=run_var)
    out["loss"] = (head or head_model.head("node", head_model.SOFTMAX, labels))(out)
    return out
