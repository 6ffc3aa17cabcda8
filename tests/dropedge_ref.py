"""Host restatement of the DropEdge contract of include/gatv2_abi.h ("DropEdge"): the per-edge keep mask in numpy (the
dropout hash, keyed 0x40000000 + layer), the CSR with the dropped edges removed, and the fp64 model of a step with one mask for all
layers: the model of tests/step_ref.py run on that reduced graph."""
import numpy as np

import step_ref
from dropout_ref import fmix32, mix, threshold  # noqa: F401  (the hash is the dropout one, bit for bit)

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


def forward(cfg, row_ptr, col_idx, labels, X, W, a, Wo, keep, attn=None, **kw):
    """fp64 step with ONE edge mask for all layers (GAT_DROPEDGE_SHARED_LAYERS) by another route than step_ref.forward(keeps=...): that
    model on the reduced graph.  attn[l] [H][E] are attention factors computed on the FULL CSR (positions k are the original ones),
    filtered by keep here; **kw goes to step_ref.forward (tests/test_dropedge_cpu.py checks that the two routes agree)."""
    rp, ci = reduce_graph(row_ptr, col_idx, keep)
    attn_r = None if attn is None else [np.asarray(f)[:, np.asarray(keep, bool)] for f in attn]
    return step_ref.forward(cfg, rp, ci, labels, X, W, a, Wo, attn=attn_r, **kw)
