"""What tests/test_neg_sampling_cpu.py and tests/test_neg_sampling.py share: the fixture graphs of the negative sampler
(include/gatv2_abi.h "negative sampling"), the brute-force acceptance rule over a Python set of edges, the cases."""
import numpy as np

N = 300
DEGREES = [0, 1, 2, 31, 32, 33, 255, 256, 257, 299]      # in-degrees of rows 0 .. 9; row 9 is the hub: every node but itself
HUB = 9
VARIANTS = ("ascending", "shuffled", "duplicates")
UNIFORM, CORRUPT = 1, 2
BOTH, SELF = 1, 2
FLAGS = (0, BOTH, SELF, BOTH | SELF)
COUNTS = (1, 63, 64, 65, 1000)
ROUNDS = (0, 1, 2 ** 40)
SEED = 0x6E6567
GRAPH_SEED = 77


def fixture_graph(pkg, variant):
    """N = 300 nodes; rows 0 .. 9 have DEGREES distinct sources (row 9 all nodes but itself), every other row 3 .. 7 (about 5) distinct
    hash-drawn sources.  "ascending": every row sorted; "shuffled": every row in its hash order (not ascending); "duplicates": the
    ascending rows with every source of every third row and the first source of every other row given twice.  -> (row_ptr, col_idx)."""
    H = pkg.synth._hash
    rows = []
    for r in range(N):
        order = np.argsort(H(GRAPH_SEED, 100 + r, np.arange(N, dtype=np.uint64)), kind="stable")
        if r == HUB:
            src = order[order != r]
        else:
            d = DEGREES[r] if r < len(DEGREES) else 3 + int(H(GRAPH_SEED, 5, np.array([r], np.uint64))[0] % np.uint64(5))
            src = order[:d]
        if variant != "shuffled":
            src = np.sort(src)
        if variant == "duplicates" and len(src):
            src = np.sort(np.concatenate([src, src if r % 3 == 0 else src[:1]]))
        rows.append(src.astype(np.int32))
    row_ptr = np.zeros(N + 1, np.int32)
    row_ptr[1:] = np.cumsum([len(s) for s in rows])
    return row_ptr, np.concatenate(rows).astype(np.int32)


def complete_graph(n):
    """Every (u, v), self-loops included: no candidate is ever accepted."""
    row_ptr = (np.arange(n + 1) * n).astype(np.int32)
    return row_ptr, np.tile(np.arange(n, dtype=np.int32), n)


def single_node():
    """N = 1 without edges: the only candidate is the self pair."""
    return np.zeros(2, np.int32), np.zeros(0, np.int32)


def edge_set(row_ptr, col_idx):
    """{(source, destination)} by brute force."""
    return {(int(col_idx[e]), r) for r in range(len(row_ptr) - 1) for e in range(row_ptr[r], row_ptr[r + 1])}


def fails(edges, u, v, flags):
    """Per pair: the acceptance rule is violated."""
    return np.array([(a == b and not flags & SELF) or (a, b) in edges or (bool(flags & BOTH) and (b, a) in edges)
                     for a, b in zip(u.tolist(), v.tolist())], bool)


def sources(pkg, row_ptr, col_idx, n_src=50):
    """Source pairs of CORRUPT: hash-drawn edges of the graph as (source, destination)."""
    u, v, _ = pkg.synth.link_pairs(row_ptr, col_idx, n_src, 0, seed=5)
    return u, v


def hub_sources(n_src=40):
    """Every source pair ends at the hub: a role-0 negative (w, HUB) is an edge for every w but the hub itself, which is the self pair."""
    return (np.arange(n_src, dtype=np.int32) * 7 + 10) % N, np.full(n_src, HUB, np.int32)


def roles(pkg, seed, round, count):
    """role = H(seed, 43, round * count + j) & 1"""
    with np.errstate(over="ignore"):
        c = np.uint64(round) * np.uint64(count) + np.arange(count, dtype=np.uint64)
    return (pkg.synth._hash(seed, 43, c) & np.uint64(1)).astype(np.int64)
