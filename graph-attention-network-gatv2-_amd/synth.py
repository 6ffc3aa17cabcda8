"""Deterministic synthetic datasets of the shapes BASELINE.json names (the real files are a
Google-Drive link in the reference's README, R:21, and there is no network).

Counter-based (splitmix64 of seed/stream/index), so any row range can be generated on any rank
and is identical everywhere.  Graph law: in-degree by largest-remainder
apportionment of exactly E edges over w_i = (pi(i)+r0)^-beta; every edge's source drawn from the
same law under an independent permutation; sources ascending inside a row; self-loops and
duplicates kept.  CSR rows are destinations, columns sources — the reference's convention
(GATv2_edge_based.cu E:74-82).
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np

GRAPH_SEED = 0x67617432
_U64 = np.uint64
_GOLD = _U64(0x9E3779B97F4A7C15)


def _mix(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64, copy=True)
    x ^= x >> _U64(30); x *= _U64(0xBF58476D1CE4E5B9)
    x ^= x >> _U64(27); x *= _U64(0x94D049BB133111EB)
    x ^= x >> _U64(31)
    return x


def _hash(seed: int, stream: int, idx: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        base = _mix(np.array([(seed ^ (stream * 0xD1342543DE82EF95)) & 0xFFFFFFFFFFFFFFFF], np.uint64))[0]
        return _mix(idx.astype(np.uint64) * _GOLD + base)


def _uniform01(seed: int, stream: int, idx: np.ndarray) -> np.ndarray:
    return (_hash(seed, stream, idx) >> _U64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _argsort_u64(keys: np.ndarray) -> np.ndarray:
    return np.argsort(keys, kind="stable")


def _perm(seed: int, stream: int, n: int, argsort=_argsort_u64) -> np.ndarray:
    """pi[i] = rank of node i under a seeded hash order."""
    order = argsort(_hash(seed, stream, np.arange(n, dtype=np.uint64)))
    pi = np.empty(n, np.int64)
    pi[order] = np.arange(n, dtype=np.int64)
    return pi


def graph_tables(n: int, e: int, seed: int = GRAPH_SEED, beta: float = 0.75, r0: float = 100.0, argsort=_argsort_u64):
    """The N-sized part of the graph law: -> (row_ptr int32[n+1], cdf float64[n] over rank weights,
    node_of_rank int32[n]).  Cheap (a few argsorts of n values); the E-sized part follows in powerlaw_graph (host)
    or gat_synth_sources_device (GPU, same arrays bit for bit).  `argsort`: stable ascending argsort of uint64 keys
    (the device generator passes one that sorts on the GPU)."""
    rank_w = (np.arange(n, dtype=np.float64) + r0) ** (-beta)        # weight by rank
    pi_in = _perm(seed, 1, n, argsort)
    w = rank_w[pi_in]
    quota = w * (e / w.sum())
    deg = np.floor(quota).astype(np.int64)
    rem = int(e - deg.sum())
    if rem > 0:
        frac = quota - deg
        # largest remainders first, ties in node order: == argsort(-frac, stable).  frac is in [0, 1): the bit
        # patterns of non-negative doubles order like the values, their complements the other way round
        top = argsort(~np.ascontiguousarray(frac).view(np.uint64))[:rem]
        deg[top] += 1
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    assert row_ptr[-1] == e
    # sources: inverse CDF over rank weights, rank -> node through an independent permutation
    pi_src = _perm(seed, 2, n, argsort)
    node_of_rank = np.empty(n, np.int64)
    node_of_rank[pi_src] = np.arange(n, dtype=np.int64)
    cdf = np.cumsum(rank_w)
    cdf /= cdf[-1]
    return row_ptr.astype(np.int32), cdf, node_of_rank.astype(np.int32)


def powerlaw_graph(n: int, e: int, seed: int = GRAPH_SEED, beta: float = 0.75, r0: float = 100.0
                   ) -> Tuple[np.ndarray, np.ndarray]:
    """-> (row_ptr int32[n+1], col_idx int32[e])"""
    row_ptr, cdf, node_of_rank = graph_tables(n, e, seed, beta, r0)
    deg = np.diff(row_ptr.astype(np.int64))
    col = np.empty(e, np.int64)
    step = 1 << 24
    for lo in range(0, e, step):
        hi = min(e, lo + step)
        u = _uniform01(seed, 3, np.arange(lo, hi, dtype=np.uint64))
        r = np.searchsorted(cdf, u, side="right")
        np.minimum(r, n - 1, out=r)
        col[lo:hi] = node_of_rank[r]
    # ascending sources inside each row: sort by (row, src)
    dst = np.repeat(np.arange(n, dtype=np.int64), deg)
    key = dst * np.int64(n) + col
    key.sort(kind="stable")
    col = (key % np.int64(n)).astype(np.int32)
    return row_ptr, col


def features(n: int, f: int, seed: int = GRAPH_SEED + 1, rows: Optional[Tuple[int, int]] = None,
             kind: str = "uniform") -> np.ndarray:
    """uniform: U[-1,1) fp32.  bow: sparse binary rows (~18 nnz) row-normalised (Cora-like)."""
    lo, hi = rows if rows is not None else (0, n)
    out = np.empty((hi - lo, f), np.float32)
    chunk = max(1, (1 << 24) // max(f, 1))
    for a in range(lo, hi, chunk):
        b = min(hi, a + chunk)
        idx = (np.arange(a, b, dtype=np.uint64)[:, None] * _U64(f) + np.arange(f, dtype=np.uint64)[None, :])
        u = _uniform01(seed, 7, idx.reshape(-1)).reshape(b - a, f)
        if kind == "bow":
            m = (u < (18.0 / f)).astype(np.float32)
            s = m.sum(axis=1, keepdims=True)
            out[a - lo:b - lo] = m / np.maximum(s, 1.0)
        else:
            out[a - lo:b - lo] = (u * 2.0 - 1.0).astype(np.float32)
    return out


def labels(n: int, c: int, seed: int = GRAPH_SEED + 2, rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    lo, hi = rows if rows is not None else (0, n)
    lab = (_hash(seed, 11, np.arange(lo, hi, dtype=np.uint64)) % _U64(c)).astype(np.int32)
    if lo == 0 and hi > 0:
        lab[0] = c - 1          # C = max(label)+1 (E:1107) must come out as requested
    return lab


# name -> (nodes, edges, features, classes, feature kind); BASELINE.json "configs"
SHAPES: Dict[str, Tuple[int, int, int, int, str]] = {
    "cora": (2708, 5429, 1433, 7, "bow"),
    "pubmed": (19717, 44338, 500, 3, "uniform"),
    "arxiv": (169343, 1166243, 128, 40, "uniform"),
    "products": (2450000, 61900000, 100, 47, "uniform"),
    "pl10m": (10000000, 250000000, 128, 47, "uniform"),
}


def make_dataset(name: str, scale: float = 1.0, seed: int = GRAPH_SEED):
    """-> dict(row_ptr, col_idx, x, labels, n, e, f, c).  scale<1 shrinks nodes and edges alike."""
    n, e, f, c, kind = SHAPES[name]
    if scale != 1.0:
        n, e = max(16, int(n * scale)), max(16, int(e * scale))
    rp, ci = powerlaw_graph(n, e, seed)
    return dict(row_ptr=rp, col_idx=ci, x=features(n, f, seed + 1, kind=kind), labels=labels(n, c, seed + 2),
                n=n, e=e, f=f, c=c, name=name)


def make_dataset_device(name: str, device, scale: float = 1.0, seed: int = GRAPH_SEED, stream: int = 0, beta: float = 0.75,
                        sorted_sources: bool = False):
    """The same dataset generated ON the GPU (csrc/gat_synth.hip): the host builds the N-sized tables, the device
    draws and sorts the E sources and fills features and labels.  -> dict(row_ptr (host int32), d_col_idx, d_x,
    d_labels (torch tensors on `device`: feed their data_ptr() to GatContext.set_*_device), n, e, f, c).  Bit-for-bit
    make_dataset's arrays (tests/test_synth_device.py)."""
    import ctypes as C
    import torch
    from . import abi
    lib = abi.load_library()
    n, e, f, c, kind = SHAPES[name]
    if scale != 1.0:
        n, e = max(16, int(n * scale)), max(16, int(e * scale))
    def device_argsort(keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        order = np.empty(len(keys), np.int32)
        abi._chk(lib.gat_synth_argsort_u64(keys.ctypes.data_as(C.c_void_p), len(keys), order.ctypes.data_as(C.c_void_p), None))
        return order

    rp, cdf, nor = graph_tables(n, e, seed, beta, argsort=device_argsort)
    if sorted_sources:          # experiment (bench.py --sorted-sources): source popularity decreasing with the node id, i.e. what a
        nor = np.arange(n, dtype=np.int32)      # library-side popularity ordering of the table rows would make of ANY graph
    d_col = torch.empty(max(e, 1), dtype=torch.int32, device=device)
    d_x = torch.empty((n, f), dtype=torch.float32, device=device)
    d_lab = torch.empty(n, dtype=torch.int32, device=device)
    st = C.c_void_p(stream or None)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    abi._chk(lib.gat_synth_sources_device(vp(cdf), vp(nor), vp(rp), n, e, seed, C.c_void_p(d_col.data_ptr()), st))
    abi._chk(lib.gat_synth_features_device(seed + 1, 0, n, f, 1 if kind == "bow" else 0, C.c_void_p(d_x.data_ptr()), st))
    abi._chk(lib.gat_synth_labels_device(seed + 2, 0, n, c, C.c_void_p(d_lab.data_ptr()), st))
    torch.cuda.synchronize(device)
    return dict(row_ptr=rp, d_col_idx=d_col[:e], d_x=d_x, d_labels=d_lab, n=n, e=e, f=f, c=c, name=name)


def write_text_dataset(ds: dict, root: str, name: Optional[str] = None) -> str:
    """Write the four whitespace text files the reference loads (R:20-27, E:1079-1099); with ds["edge_features"] ([E][Fe], rows in CSR
    order) also edge_features.txt, which train_edge --edge-features reads."""
    d = os.path.join(root, name or ds["name"])
    os.makedirs(d, exist_ok=True)
    np.savetxt(os.path.join(d, "features.txt"), ds["x"], fmt="%.9g")
    np.savetxt(os.path.join(d, "row_ptr.txt"), ds["row_ptr"], fmt="%d")
    np.savetxt(os.path.join(d, "col_idx.txt"), ds["col_idx"], fmt="%d")
    np.savetxt(os.path.join(d, "labels.txt"), ds["labels"], fmt="%d")
    if ds.get("targets") is not None:           # train_edge --loss bce|mse: rows of C floats, nan = missing
        np.savetxt(os.path.join(d, "targets.txt"), np.asarray(ds["targets"]), fmt="%.9g")
    if ds.get("edge_features") is not None:
        np.savetxt(os.path.join(d, "edge_features.txt"), np.asarray(ds["edge_features"]).reshape(len(ds["col_idx"]), -1), fmt="%.9g")
    return d


def edge_features(seed: int, n_edges: int, fe: int) -> np.ndarray:
    """Deterministic per-edge attributes [n_edges][fe] (fp32, standard normal) for the tests and tools of the edge-feature path
    (gatv2_abi.h "edge features"): row j belongs to CSR edge j.  A function of (seed, n_edges, fe) alone."""
    if n_edges < 0 or fe < 1:
        raise ValueError(f"edge_features: bad sizes (n_edges={n_edges}, fe={fe})")
    rng = np.random.default_rng([int(seed) & (2 ** 63 - 1), 0xEA])
    return rng.standard_normal((int(n_edges), int(fe))).astype(np.float32)


def targets(kind: str, n_rows: int, n_cols: int, seed: int = GRAPH_SEED + 3, missing: float = 0.0) -> np.ndarray:
    """Float targets [n_rows][n_cols] for the BCE / MSE heads (gatv2_abi.h "loss modes of the output head"), hash-drawn per entry:
    kind "multilabel": 0 / 1 with probability 1/2 each; "regression": U[-1,1).  A `missing` fraction of the entries (a second hash
    stream, each entry independently) is NaN.  A function of the arguments alone."""
    if kind not in ("multilabel", "regression"):
        raise ValueError(f"targets: kind must be 'multilabel' or 'regression', got {kind!r}")
    if n_rows < 0 or n_cols < 1 or not 0.0 <= missing <= 1.0:
        raise ValueError(f"targets: bad arguments (n_rows={n_rows}, n_cols={n_cols}, missing={missing})")
    idx = np.arange(int(n_rows) * int(n_cols), dtype=np.uint64)
    u = _uniform01(seed, 13, idx)
    t = (u < 0.5).astype(np.float32) if kind == "multilabel" else (u * 2.0 - 1.0).astype(np.float32)
    if missing > 0.0:
        t[_uniform01(seed, 17, idx) < missing] = np.nan
    return t.reshape(int(n_rows), int(n_cols))


def link_pairs(row_ptr, col_idx, n_pos: int, n_neg: int, seed: int = GRAPH_SEED + 4):
    """Node pairs for the pair head (gatv2_abi.h "pair head"): n_pos positives drawn (with replacement) from the graph's own edges —
    pair (source, destination) of a hash-drawn CSR edge, t = 1 — then n_neg negatives, uniform node pairs with t = 0 (not filtered
    against the edges: on a sparse graph a drawn pair is an edge with probability E / N^2).  Hash-drawn per pair with the generators'
    counter hash: a function of the arguments alone.  -> (u [P] int32, v [P] int32, t [P] float32), P = n_pos + n_neg."""
    rp, ci = np.asarray(row_ptr, np.int64), np.asarray(col_idx, np.int64)
    n, e = len(rp) - 1, len(ci)
    if n_pos < 0 or n_neg < 0 or n < 1 or (n_pos > 0 and e < 1):
        raise ValueError(f"link_pairs: bad arguments (n_pos={n_pos}, n_neg={n_neg}, {n} nodes, {e} edges)")
    pe = (_hash(seed, 19, np.arange(n_pos, dtype=np.uint64)) % _U64(max(e, 1))).astype(np.int64)
    pos_v = np.searchsorted(rp, pe, side="right") - 1            # the destination row of edge pe
    idx = np.arange(n_neg, dtype=np.uint64)
    neg_u = (_hash(seed, 23, idx) % _U64(n)).astype(np.int64)
    neg_v = (_hash(seed, 29, idx) % _U64(n)).astype(np.int64)
    u = np.concatenate([ci[pe], neg_u]).astype(np.int32)
    v = np.concatenate([pos_v, neg_v]).astype(np.int32)
    t = np.concatenate([np.ones(n_pos, np.float32), np.zeros(n_neg, np.float32)])
    return u, v, t


NEG_UNIFORM, NEG_CORRUPT = 1, 2                      # gatv2_abi.h GAT_NEG_*
NEG_BOTH_DIRECTIONS, NEG_ALLOW_SELF = 1, 2
NEG_TRIES = 16


def negative_pairs(row_ptr, col_idx, mode: int, count: int, seed: int, round: int, flags: int = 0, src_u=None, src_v=None):
    """The sampling law of gatv2_abi.h "negative sampling" in numpy — what gat_resample_negatives / gat_op_negative_sample draw, bit
    for bit.  Negative j in [0, count), attempt a in [0, 16): counter k = (round * count + j) * 16 + a (wrapping uint64).
    NEG_UNIFORM: u = H(seed, 37, k) % N, v = H(seed, 41, k) % N.  NEG_CORRUPT: source pair p = j % n_src, role = H(seed, 43,
    round * count + j) & 1 once per negative, w = H(seed, 37, k) % N; role 0: (w, v_p), role 1: (u_p, w).  Accepted: u != v (unless
    NEG_ALLOW_SELF), (u, v) not an edge — u not among the sources of row v — nor, with NEG_BOTH_DIRECTIONS, (v, u).  The first accepted
    attempt wins; a negative without one keeps attempt 15's candidate and counts as unfiltered.
    -> (u [count] int32, v [count] int32, unfiltered)."""
    rp, ci = np.asarray(row_ptr, np.int64), np.asarray(col_idx, np.int64)
    n = len(rp) - 1
    if mode not in (NEG_UNIFORM, NEG_CORRUPT) or flags & ~(NEG_BOTH_DIRECTIONS | NEG_ALLOW_SELF) or count < 1 or n < 1:
        raise ValueError(f"negative_pairs: bad arguments (mode={mode}, flags={flags}, count={count}, {n} nodes)")
    corrupt = mode == NEG_CORRUPT
    if corrupt:
        if src_u is None or src_v is None or len(src_u) < 1 or len(src_u) != len(src_v):
            raise ValueError("negative_pairs: NEG_CORRUPT needs at least one source pair")
        su, sv = np.asarray(src_u, np.int64), np.asarray(src_v, np.int64)
    edges = np.unique(np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) * n + ci)      # sorted keys dst * N + src

    def is_edge(a, b):                                   # (a, b) is an edge: a among the sources of row b
        key = b * n + a
        pos = np.searchsorted(edges, key)
        return (pos < len(edges)) & (edges[np.minimum(pos, max(len(edges) - 1, 0))] == key) if len(edges) else np.zeros(len(a), bool)

    nn = _U64(n)
    with np.errstate(over="ignore"):
        c = _U64(int(round) & 0xFFFFFFFFFFFFFFFF) * _U64(count) + np.arange(count, dtype=np.uint64)
    if corrupt:
        p = np.arange(count, dtype=np.int64) % len(su)
        role = (_hash(seed, 43, c) & _U64(1)).astype(np.int64)
    u, v = np.zeros(count, np.int64), np.zeros(count, np.int64)
    done = np.zeros(count, bool)
    for a in range(NEG_TRIES):
        with np.errstate(over="ignore"):
            k = c * _U64(NEG_TRIES) + _U64(a)
        if corrupt:
            w = (_hash(seed, 37, k) % nn).astype(np.int64)
            cu, cv = np.where(role == 0, w, su[p]), np.where(role == 0, sv[p], w)
        else:
            cu, cv = (_hash(seed, 37, k) % nn).astype(np.int64), (_hash(seed, 41, k) % nn).astype(np.int64)
        ok = ~is_edge(cu, cv)
        if not flags & NEG_ALLOW_SELF:
            ok &= cu != cv
        if flags & NEG_BOTH_DIRECTIONS:
            ok &= ~is_edge(cv, cu)
        u[~done], v[~done] = cu[~done], cv[~done]          # the candidate of the first accepted attempt, else of the last
        done |= ok
    return u.astype(np.int32), v.astype(np.int32), int((~done).sum())


def graph_batch(n_graphs: int, nodes_lo: int, nodes_hi: int, avg_degree: float, seed: int = GRAPH_SEED, f: int = 32, c: int = 4):
    """A batch of n_graphs small graphs (molecule-like) packed block-diagonally into one CSR, for the graph-level readout
    (gatv2_abi.h "graph-level readout"): graph g has a size drawn uniformly from [nodes_lo, nodes_hi] and owns the contiguous nodes
    graph_ptr[g] .. graph_ptr[g+1]-1; every node gets one self-loop plus Poisson(avg_degree - 1) in-edges from uniformly drawn nodes of
    its own graph, sources ascending inside a row (rows = destinations).  Features are `features(n, f)`, the labels — one per GRAPH —
    `labels(n_graphs, c)`.  A function of the arguments alone.
    -> dict(row_ptr, col_idx, graph_ptr, x, labels [n_graphs], n, e, f, c, n_graphs)."""
    if n_graphs < 1 or nodes_lo < 1 or nodes_hi < nodes_lo or avg_degree < 1.0:
        raise ValueError(f"graph_batch: bad arguments (n_graphs={n_graphs}, nodes {nodes_lo}..{nodes_hi}, avg_degree={avg_degree})")
    rng = np.random.default_rng([int(seed) & (2 ** 63 - 1), 0x6B])
    sizes = rng.integers(nodes_lo, nodes_hi + 1, n_graphs)
    graph_ptr = np.zeros(n_graphs + 1, np.int64)
    graph_ptr[1:] = np.cumsum(sizes)
    n = int(graph_ptr[-1])
    if n >= 2 ** 31 - 1:
        raise ValueError("graph_batch: the node count does not fit int32")
    first = np.repeat(graph_ptr[:-1], sizes)                  # first node of the node's graph
    size = np.repeat(sizes, sizes)
    deg = 1 + rng.poisson(avg_degree - 1.0, n)
    row_ptr = np.zeros(n + 1, np.int64)
    row_ptr[1:] = np.cumsum(deg)
    e = int(row_ptr[-1])
    if e > 2 ** 31 - 1:
        raise ValueError("graph_batch: the edge count does not fit int32")
    dst = np.repeat(np.arange(n, dtype=np.int64), deg)
    src = first[dst] + (rng.random(e) * size[dst]).astype(np.int64)
    src[row_ptr[:-1]] = np.arange(n)                          # the first edge of every row is its self-loop
    src = src[np.lexsort((src, dst))]                         # ascending inside a row (dst is sorted already)
    return dict(row_ptr=row_ptr.astype(np.int32), col_idx=src.astype(np.int32), graph_ptr=graph_ptr.astype(np.int32),
                x=features(n, f, seed + 1), labels=labels(n_graphs, c, seed + 2), n=n, e=e, f=f, c=c, n_graphs=n_graphs,
                name=f"graph_batch_{n_graphs}")
