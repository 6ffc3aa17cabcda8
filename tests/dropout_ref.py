"""Host restatement of the dropout contract of include/gatv2_abi.h ("dropout"): the counter-based mask hash in numpy,
and an fp64 torch autograd model of the GATv2 step with those masks applied (tests/torch_ref.py plus dropout)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, np.uint64) & M32


def fmix32(h):
    h = _u32(h)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def mix(k, v):
    return fmix32(_u32(k) ^ ((_u32(v) * np.uint64(0x9E3779B9) + np.uint64(0x7F4A7C15)) & M32))


def key(seed, step, layer, kind):
    """K(kind, l); kind 0 = feature, 1 = attention."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    k = mix(seed & 0xFFFFFFFF, seed >> 32)
    k = mix(k, step & 0xFFFFFFFF)
    k = mix(k, step >> 32)
    return mix(k, 2 * layer + kind)


def threshold(p):
    return min(1 << 24, int(np.floor(np.float64(np.float32(p)) * 2.0 ** 24 + 0.5)))


def scale(p):
    return np.float32(1.0 / (1.0 - np.float64(np.float32(p))))


def keep(r, p):
    return (_u32(r) >> np.uint64(8)) >= np.uint64(threshold(p))


def attn_factor(seed, step, layer, row_ptr, H, p, nodes=None):
    """[H][E] kappa*s_a per (head, CSR edge); nodes[row] = unsharded id of the row (default: the row index)."""
    row_ptr = np.asarray(row_ptr, np.int64)
    deg = np.diff(row_ptr)
    rows = np.repeat(np.arange(len(deg)), deg)
    node = rows if nodes is None else np.asarray(nodes, np.int64)[rows]
    kpos = np.arange(row_ptr[-1]) - row_ptr[rows]
    kn = mix(mix(key(seed, step, layer, 1), node), kpos)
    out = np.empty((H, len(rows)), np.float32)
    for h in range(H):
        out[h] = np.where(keep(mix(kn, h), p), scale(p), np.float32(0))
    return out


def feat_factor(seed, step, layer, n_rows, F, p, nodes=None):
    """[rows][F] kappa*s_f of a layer's input."""
    node = np.arange(n_rows) if nodes is None else np.asarray(nodes, np.int64)
    kn = mix(key(seed, step, layer, 0), node)[:, None]
    r = mix(kn, np.arange(F)[None, :])
    return np.where(keep(r, p), scale(p), np.float32(0)).astype(np.float32)


def _nonzero_min(t):
    """smallest |value| that is not exactly 0 (exact zeros — empty rows, dropped terms — take the same LeakyReLU' branch on
    both sides: max(x, slope*x) and x > 0)"""
    v = t.detach().abs()
    v = v[v > 0]
    return float(v.min()) if v.numel() else np.inf


def forward(cfg, row_ptr, col_idx, labels, X, W, a, Wo, attn=None, feat=None, slope=0.01, bf16_pl=False):
    """fp64 autograd step with masks: attn[l] [H][E], feat[l] [N][F_l] (None: no dropout of that kind).
    bf16_pl: the gathered table PL is used rounded to bf16 (nearest even) with a straight-through gradient — what bf16 storage
    computes; without it, bf16 rounding of PL moves scores across the LeakyReLU kink and the gradients differ by a few %.
    -> dict(loss, hpre[l], s_min, hpre_min, W, a, Wo leaf tensors)."""
    import torch
    dt = torch.float64
    N = len(row_ptr) - 1
    deg = np.diff(row_ptr)
    dst = torch.from_numpy(np.repeat(np.arange(N), deg)).long()
    src = torch.from_numpy(np.asarray(col_idx)).long()
    Wt = torch.tensor(np.asarray(W), dtype=dt, requires_grad=True)
    at = torch.tensor(np.asarray(a), dtype=dt, requires_grad=True)
    Wot = torch.tensor(np.asarray(Wo), dtype=dt, requires_grad=True)
    x = torch.tensor(np.asarray(X), dtype=dt)
    out = {"hpre": [], "W": Wt, "a": at, "Wo": Wot, "s_min": np.inf, "hpre_min": np.inf}
    for l in range(cfg.L):
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
        out["s_min"] = min(out["s_min"], _nonzero_min(s))
        e = (al * torch.nn.functional.leaky_relu(s, slope)).sum(-1)              # [E,H]
        m = torch.full((N, H), -1e9, dtype=dt).scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
        pe = torch.exp(e - m[dst])
        Z = torch.zeros((N, H), dtype=dt).index_add(0, dst, pe)
        alpha = pe / (Z[dst] + 1e-8)
        w = alpha if attn is None else alpha * torch.from_numpy(np.asarray(attn[l], np.float64).T)
        hpre = torch.zeros((N, H, D), dtype=dt).index_add(0, dst, w[..., None] * PL[src])
        out["hpre_min"] = min(out["hpre_min"], _nonzero_min(hpre))
        act = torch.nn.functional.leaky_relu(hpre, slope)
        x = act.mean(1) if l == cfg.L - 1 else act.reshape(N, H * D)
        out["hpre"].append(hpre)
    z = x @ Wot.view(cfg.num_classes, cfg.outdims[-1]).t()
    ez = torch.exp(z - z.max(dim=1, keepdim=True).values.detach())
    y = ez / (ez.sum(1, keepdim=True) + 1e-8)
    lab = torch.from_numpy(np.asarray(labels)).long()
    out["loss"] = -torch.log(torch.clamp(y[torch.arange(N), lab], min=1e-12)).sum()
    return out
