"""The cases of the ranking-metrics tests (tests/test_rank_metrics.py on the GPU, tests/test_rank_metrics_cpu.py on the host): the seam's
inputs and the four contexts.  Everything is a function of fixed seeds; the CPU test asserts on these very arrays the conditions the GPU
tests rely on (which columns have both classes, the tie groups, the saturated column)."""
import functools

import numpy as np

ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 20000)
COLS = (1, 3, 47)
LAWS = ("continuous", "quant8", "equal")
INPUTS = ("labels", "targets", "targets_nan")
KS8 = (1, 2, 3, 5, 10, 50, 100, 1000)
SENTINEL = np.float32(-12345.0)
PAD = 3                                          # floats behind a row when score_stride > n_cols


def _scores(rng, rows, cols, law):
    if law == "continuous":
        return rng.standard_normal((rows, cols)).astype(np.float32)
    if law == "quant8":                          # 8 values: tie groups of rows / 8 entries, across every block boundary
        return (rng.integers(0, 8, (rows, cols)).astype(np.float32) - 3.0) / 4.0
    return np.full((rows, cols), 0.75, np.float32)


def _supervision(rng, rows, cols, kind):
    if kind == "labels":
        return rng.integers(0, cols, rows).astype(np.int32), None
    t = (rng.random((rows, cols)) > 0.6).astype(np.float32)
    if kind == "targets_nan":
        t[rng.random((rows, cols)) < 0.2] = np.nan
    return None, t


def _case(name, seed, rows, cols, law, kind, masked, padded, edit=None):
    rng = np.random.default_rng(seed)
    s = _scores(rng, rows, cols, law)
    labels, targets = _supervision(rng, rows, cols, kind)
    mask = (rng.random(rows) > 0.3) if masked else None
    case = dict(name=name, rows=rows, cols=cols, law=law, kind=kind, scores=s, labels=labels, targets=targets, mask=mask,
                stride=cols + (PAD if padded else 0), tie_heavy=False, saturated=law == "equal", specials=False, degenerate=False)
    if edit is not None:
        edit(case, rng)
    return case


def _specials(case, rng):
    """-0.0 against +0.0, subnormals, +-inf and NaN scores, each on both classes of every column."""
    s = case["scores"]
    vals = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf, np.nan], np.float32)
    special = vals[rng.integers(0, len(vals), s.shape)]
    case["scores"] = np.where(rng.random(s.shape) < 0.2, s, special).astype(np.float32)       # a fifth stays continuous
    case["specials"] = True


def _degenerate(case, rng):
    """column 0 without positives, column 1 without negatives (among the present targets)."""
    t = case["targets"]
    t[:, 0] = np.where(np.isnan(t[:, 0]), np.nan, 0.0)
    t[:, 1] = np.where(np.isnan(t[:, 1]), np.nan, 1.0)
    case["degenerate"] = True


@functools.lru_cache(maxsize=None)
def seam_cases():
    out = []
    i = 0
    for rows in ROWS:
        for cols in COLS:
            law = LAWS[i % 3] if rows < 20000 else "continuous"
            kind = INPUTS[(i // 3 + i) % 3] if (rows, cols) != (20000, 47) else "labels"       # (the brute force of the CPU twin stays quick)
            out.append(_case(f"r{rows}-c{cols}-{law}-{kind}-{'mask' if i % 2 else 'all'}-{'pad' if i % 4 < 2 else 'dense'}", 100 + i, rows, cols,
                             law, kind, bool(i % 2), i % 4 < 2))
            i += 1
    for cols in COLS:                                # tie-heavy: groups of ~2500 with both classes
        kind = "targets_nan" if cols < 47 else "labels"
        out.append(_case(f"ties-r20000-c{cols}", 200 + cols, 20000, cols, "quant8", kind, cols == 3, cols == 1))
        out[-1]["tie_heavy"] = True
    out.append(_case("saturated-r20000-c1", 300, 20000, 1, "equal", "targets", False, False))
    out.append(_case("saturated-r1000-c3-mask", 301, 1000, 3, "equal", "targets_nan", True, True))
    out.append(_case("specials-r257-c3", 302, 257, 3, "continuous", "targets", False, True, edit=_specials))
    out.append(_case("specials-r1000-c1-mask", 303, 1000, 1, "continuous", "targets_nan", True, False, edit=_specials))
    out.append(_case("degenerate-r257-c3", 304, 257, 3, "continuous", "targets_nan", True, False, edit=_degenerate))
    out.append(_case("degenerate-r64-c47-quant", 305, 64, 47, "quant8", "targets", False, True, edit=_degenerate))
    out.append(_case("labels-mask-r1000-c3", 306, 1000, 3, "quant8", "labels", True, True))
    return tuple(out)


def seam_ids():
    return [c["name"] for c in seam_cases()]


def case_ks(case, n_neg0):
    """The K of a case's first call: 1 and the three around column 0's negative count (clipped to K >= 1)."""
    return tuple(max(1, int(k)) for k in (1, n_neg0 - 1, n_neg0, n_neg0 + 1))


def padded(case):
    """scores as the seam takes them: rows `stride` floats apart, SENTINEL behind every row."""
    buf = np.full((case["rows"], case["stride"]), SENTINEL, np.float32)
    buf[:, :case["cols"]] = case["scores"]
    return buf


# -- the four contexts: (name, what the head's rows are, loss) on feature_cases.parity_graph
CONTEXTS = ("pair_bce", "node_softmax", "node_bce_nan", "readout_softmax")
CTX_KS = (1, 3, 10, 50)
HEADS, OUTDIMS = [8, 8], [8, 8]
PARAM_SEED = 7
N_POS, N_NEG = 180, 220                          # the pair head's list: positives first, then the negative slots
N_GRAPHS = 31                                    # the readout's graphs: 30 of five nodes and an empty one


@functools.lru_cache(maxsize=None)
def context_case(name):
    """-> dict(g, kind, C, rows, labels | targets, mask, and what the kind needs).  Supervision and mask do not depend on the device."""
    import __graft_entry__ as entry
    import feature_cases as FC
    import loss_ref as LR
    pkg = entry.load_package()
    g = FC.parity_graph()
    n = g["n"]
    rng = np.random.default_rng(77)
    if name == "pair_bce":
        u, v, t = pkg.synth.link_pairs(g["row_ptr"], g["col_idx"], N_POS, N_NEG, seed=2)
        rows = len(u)
        return dict(name=name, g=dict(g, c=1), C=1, rows=rows, u=u, v=v, labels=None, targets=np.asarray(t, np.float32).reshape(rows, 1),
                    mask=rng.random(rows) > 0.25)
    if name == "node_softmax":
        return dict(name=name, g=g, C=g["c"], rows=n, labels=g["labels"], targets=None, mask=rng.random(n) > 0.25)
    if name == "node_bce_nan":
        T = LR.targets_for(pkg, LR.BCE, n, g["c"])
        return dict(name=name, g=g, C=g["c"], rows=n, labels=None, targets=np.asarray(T, np.float32), mask=rng.random(n) > 0.25)
    assert name == "readout_softmax"
    gp = np.concatenate([[0, 0], np.arange(1, N_GRAPHS) * (n // (N_GRAPHS - 1))]).astype(np.int32)
    gp[-1] = n
    glab = (np.arange(N_GRAPHS) % g["c"]).astype(np.int32)
    mask = np.ones(N_GRAPHS, bool)
    mask[[2, 17]] = False
    return dict(name=name, g=g, C=g["c"], rows=N_GRAPHS, graph_ptr=gp, labels=glab, targets=None, mask=mask)


def make_context(pkg, cc, **kw):
    """The context of a case, parameters from the device's own initialiser, gradients zeroed."""
    g = cc["g"]
    ctx = pkg.GatContext(HEADS, OUTDIMS, g["f"], cc["C"], **kw)
    if cc["targets"] is not None:
        ctx.set_loss("bce")
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    if cc["name"] == "pair_bce":
        ctx.set_pairs("mul", cc["u"], cc["v"])
    if cc["name"] == "readout_softmax":
        ctx.set_readout("mean", graph_ptr=cc["graph_ptr"])
    if cc["targets"] is not None:
        ctx.set_targets(cc["targets"])
    else:
        ctx.set_labels(cc["labels"])
    ctx.params_init(PARAM_SEED)
    if cc["name"] == "pair_bce":                 # sampled negatives: the slots behind the positives, drawn once
        ctx.set_negative_sampling("uniform", N_POS, cc["rows"] - N_POS, both_directions=True, seed=5)
        ctx.resample_negatives(1)
    ctx.zero_grad()
    return ctx
