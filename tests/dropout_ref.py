"""Host restatement of the dropout contract of include/gatv2_abi.h ("dropout"): the counter-based mask hash in numpy.  The fp64
model of a step that applies these masks is tests/step_ref.py."""
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
