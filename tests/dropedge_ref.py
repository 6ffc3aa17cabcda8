"""Host restatement of the DropEdge contract of include/gatv2_abi.h ("DropEdge"): the per-edge keep mask in numpy (the
dropout hash, keyed 0x40000000 + layer), the CSR with the dropped edges removed, and the fp64 model of a step: the dropout
model of tests/dropout_ref.py run on that reduced graph."""
import numpy as np

from dropout_ref import fmix32, mix, threshold  # noqa: F401  (the hash is the dropout one, bit for bit)
import dropout_ref as R

EDGE_KEY = 0x40000000


def edge_key(seed, step, layer, shared=False):
    """K_e(l): the four-mix chain over (seed lo, seed hi, step lo, step hi), then 0x40000000 + l (l = 0 when shared)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    k = mix(seed & 0xFFFFFFFF, seed >> 32)
    k = mix(k, step & 0xFFFFFFFF)
    k = mix(k, step >> 32)
    return mix(k, EDGE_KEY + (0 if shared else int(layer)))


def edge_draw(seed, step, layer, row_ptr, shared=False, nodes=None):
    """[E] the 24-bit draws r >> 8 of every CSR edge."""
    row_ptr = np.asarray(row_ptr, np.int64)
    deg = np.diff(row_ptr)
    rows = np.repeat(np.arange(len(deg)), deg)
    node = rows if nodes is None else np.asarray(nodes, np.int64)[rows]
    kpos = np.arange(row_ptr[-1]) - row_ptr[rows]
    r = mix(mix(edge_key(seed, step, layer, shared), node), kpos)
    return (np.asarray(r, np.uint64) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)


def edge_keep(seed, step, layer, row_ptr, col_idx, p, keep_self=False, shared=False, nodes=None, table_row0=0):
    """[E] bool: CSR edge kept.  nodes[row] = unsharded id of the row (default: the row index); keep_self: an edge whose
    col_idx equals table_row0 + row is never dropped."""
    row_ptr = np.asarray(row_ptr, np.int64)
    keep = edge_draw(seed, step, layer, row_ptr, shared, nodes) >= np.uint64(threshold(p))
    if keep_self:
        rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
        keep = keep | (np.asarray(col_idx, np.int64) == int(table_row0) + rows)
    return keep


def reduce_graph(row_ptr, col_idx, keep):
    """The CSR with the dropped edges removed (order inside the rows unchanged)."""
    row_ptr = np.asarray(row_ptr, np.int64)
    keep = np.asarray(keep, bool)
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    deg = np.bincount(rows[keep], minlength=len(row_ptr) - 1)
    rp = np.zeros(len(row_ptr), np.int32)
    rp[1:] = np.cumsum(deg)
    return rp, np.ascontiguousarray(np.asarray(col_idx, np.int32)[keep])


def forward(cfg, row_ptr, col_idx, labels, X, W, a, Wo, keep, attn=None, feat=None, slope=0.01, bf16_pl=False):
    """fp64 step with ONE edge mask for all layers (GAT_DROPEDGE_SHARED_LAYERS): dropout_ref.forward on the reduced graph.
    attn[l] [H][E] are attention factors computed on the FULL CSR (positions k are the original ones), filtered by keep here."""
    rp, ci = reduce_graph(row_ptr, col_idx, keep)
    attn_r = None if attn is None else [np.asarray(f)[:, np.asarray(keep, bool)] for f in attn]
    return R.forward(cfg, rp, ci, labels, X, W, a, Wo, attn=attn_r, feat=feat, slope=slope, bf16_pl=bf16_pl)


def forward_layers(cfg, row_ptr, col_idx, labels, X, W, a, Wo, keeps, attn=None, feat=None, slope=0.01, bf16_pl=False):
    """The same model with a mask PER LAYER (keeps[l] [E]): every layer aggregates over its own reduced graph.  Equal to
    forward() when all masks are the same (tests/test_dropedge_cpu.py checks that)."""
    import torch
    dt = torch.float64
    N = len(row_ptr) - 1
    dst_all = np.repeat(np.arange(N), np.diff(row_ptr))
    Wt = torch.tensor(np.asarray(W), dtype=dt, requires_grad=True)
    at = torch.tensor(np.asarray(a), dtype=dt, requires_grad=True)
    Wot = torch.tensor(np.asarray(Wo), dtype=dt, requires_grad=True)
    x = torch.tensor(np.asarray(X), dtype=dt)
    out = {"hpre": [], "W": Wt, "a": at, "Wo": Wot, "s_min": np.inf, "hpre_min": np.inf}
    for l in range(cfg.L):
        k = np.asarray(keeps[l], bool)
        dst = torch.from_numpy(dst_all[k]).long()
        src = torch.from_numpy(np.asarray(col_idx)[k]).long()
        H, D, F = cfg.heads[l], cfg.outdims[l], cfg.in_dims[l]
        if feat is not None:
            x = x * torch.from_numpy(np.asarray(feat[l], np.float64))
        Wl = Wt[cfg.w_offsets[l]:cfg.w_offsets[l + 1]].view(H, D, 2 * F)
        al = at[cfg.a_offsets[l]:cfg.a_offsets[l + 1]].view(H, D)
        PL = torch.einsum("nf,hkf->nhk", x, Wl[:, :, :F])
        PR = torch.einsum("nf,hkf->nhk", x, Wl[:, :, F:])
        if bf16_pl:                              # as dropout_ref.forward: the gathered table rounded to bf16, straight-through gradient
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
        out["hpre_min"] = min(out["hpre_min"], R._nonzero_min(hpre))
        act = torch.nn.functional.leaky_relu(hpre, slope)
        x = act.mean(1) if l == cfg.L - 1 else act.reshape(N, H * D)
        out["hpre"].append(hpre)
    z = x @ Wot.view(cfg.num_classes, cfg.outdims[-1]).t()
    ez = torch.exp(z - z.max(dim=1, keepdim=True).values.detach())
    y = ez / (ez.sum(1, keepdim=True) + 1e-8)
    lab = torch.from_numpy(np.asarray(labels)).long()
    out["loss"] = -torch.log(torch.clamp(y[torch.arange(N), lab], min=1e-12)).sum()
    return out
