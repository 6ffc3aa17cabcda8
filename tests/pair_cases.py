"""Every pair of step features on one row of a table (tests/test_feature_pairs.py on the GPU, tests/test_feature_pairs_cpu.py on the
host): the sixteen factors of a training step with their levels, the pairs the library refuses (CONSTRAINTS), a deterministic greedy
generator of a strength-2 covering array over them, the array it gives committed as the literal table ROWS (49 rows: every pair of levels
of two different factors is in a row, or is a constraint), and ONE builder from a row to everything it runs on: the graph, the
parameter groups, the supervision, the keyword arguments of tests/step_ref.py::forward with the head of tests/head_model.py, and the
context with the gat_set_* calls in the order the header requires.

A row carries, behind its sixteen levels, the first Xavier seed below bn_cases.SEEDS whose fp64 model is clear of the LeakyReLU kinks
(clear()) and the graph it runs on: "parity" (feature_cases.parity_graph; wide_graph where a layer has H*D >= 128) or, where no seed
below 400 is clear there, "small" (feature_cases.host_graph).  A plain module: the test modules import it, never each other."""
import functools

import numpy as np

import bn_cases as BC
import dropedge_ref as E
import dropout_ref as R
import edge_feat_ref as EF
import feature_cases as FC
import head_mlp_ref as HM
import head_model as HD
import loss_ref as LR
import pair_ref as PR
import readout_ref as RR
import step_ref as SR

REG = FC.REG
UNSUPPORTED = 10004

# -- the factors, in a fixed order; the first level of each is the plain one
FACTORS = (
    ("family", ("records_d8", "records_d4", "msg_rows_d16", "hd16", "generic", "hd128_generic")),
    ("dtype", ("fp32", "bf16")),
    ("keep_taps", ("taps_off", "taps_on")),
    ("layers", ("L2", "L1", "L3")),
    ("norm", ("norm_none", "layer", "layer_skip", "batch", "batch_skip")),
    ("residual", ("res_none", "linear", "bias", "both")),
    ("feat_drop", ("pf_0", "pf_on")),
    ("attn_drop", ("pa_0", "pa_on")),
    ("dropedge", ("pe_0", "pe_on", "pe_keep_self", "pe_shared")),
    ("edge_feat", ("fe0", "fe3", "fe8")),
    ("head", ("node", "readout_mean", "readout_sum", "readout_max", "pair_mul", "pair_add")),
    ("loss", ("softmax", "bce", "mse")),
    ("hidden", ("hid_off", "hid16_relu", "hid5_lrelu")),
    ("mask", ("mask_off", "mask_on")),
    ("flat", ("flat_off", "flat_on")),
    ("path", ("step", "fwd_bwd", "phases", "replay")),
)
NAMES = tuple(f[0] for f in FACTORS)
INDEX = {n: i for i, n in enumerate(NAMES)}
PLAIN = tuple(f[1][0] for f in FACTORS)                  # records_d8 / fp32 / softmax / node / gat_step: the row GAT_FUSE_LAST=1 fuses


def _flat(call, levels, text):
    return [(("flat", "flat_on"), (f, lv), call, UNSUPPORTED, text) for f, lvs in levels for lv in lvs]


# -- what the library refuses: (level, level, the call that refuses, its error code, a fragment of its message).  Nothing else is a
# constraint.  flat_lrelu_index has the head write the last layer's g itself, which only the plain node softmax head does; bf16 storage
# needs every layer on the wave-per-row kernels, and the context is refused by the call that completes it (here gat_set_labels).
CONSTRAINTS = (
    _flat("set_norm", [("norm", ("layer", "layer_skip"))], "gat_set_norm: not with flat_lrelu_index")
    + _flat("set_batch_norm", [("norm", ("batch", "batch_skip"))], "gat_set_batch_norm: not with flat_lrelu_index")
    + _flat("set_head_hidden", [("hidden", ("hid16_relu", "hid5_lrelu"))], "gat_set_head_hidden: not with flat_lrelu_index")
    + _flat("set_readout", [("head", ("readout_mean", "readout_sum", "readout_max"))], "gat_set_readout: not with flat_lrelu_index")
    + _flat("set_pairs", [("head", ("pair_mul", "pair_add"))], "gat_set_pairs: not with flat_lrelu_index")
    + _flat("set_loss", [("loss", ("bce", "mse"))], "gat_set_loss: not with flat_lrelu_index")
    + [(("dtype", "bf16"), ("family", fam), "set_labels", UNSUPPORTED, "bf16 storage needs every layer on the wave-per-row path")
       for fam in ("generic", "hd128_generic")]
)
_REFUSED = {frozenset((c[0], c[1])) for c in CONSTRAINTS}


def refused(a, b):
    """(factor, level), (factor, level) -> the pair is a constraint."""
    return frozenset((a, b)) in _REFUSED


def all_pairs():
    """Every pair of levels of two different factors that is not a constraint, in the fixed order."""
    out = []
    for i, (fi, li) in enumerate(FACTORS):
        for fj, lj in FACTORS[i + 1:]:
            out += [((fi, a), (fj, b)) for a in li for b in lj if not refused((fi, a), (fj, b))]
    return out


def row_pairs(levels):
    return [((NAMES[i], levels[i]), (NAMES[j], levels[j])) for i in range(len(NAMES)) for j in range(i + 1, len(NAMES))]


def generate():
    """The covering array: PLAIN first, then, while a pair is uncovered, the best of a few candidate rows.  A candidate starts from one of
    the first uncovered pairs and takes, factor by factor in the fixed order, the level that covers the most uncovered pairs with the
    levels already chosen and is refused with none of them (ties: the earlier level).  Every factor has a level no constraint names, so
    a row can always be finished.  No random state."""
    uncovered = set(all_pairs())
    order = all_pairs()
    rows = []

    def take(levels):
        rows.append(tuple(levels))
        uncovered.difference_update(row_pairs(levels))

    def candidate(seed_pair):
        chosen = dict(seed_pair)
        for name, lvls in FACTORS:
            if name in chosen:
                continue
            best, best_gain = None, -1
            for lv in lvls:
                if any(refused((name, lv), kv) for kv in chosen.items()):
                    continue
                gain = sum(1 for kv in chosen.items()
                           if (((name, lv), kv) if INDEX[name] < INDEX[kv[0]] else (kv, (name, lv))) in uncovered)
                if gain > best_gain:
                    best, best_gain = lv, gain
            chosen[name] = best
        levels = tuple(chosen[n] for n in NAMES)
        return levels, sum(1 for p in row_pairs(levels) if p in uncovered)
    take(PLAIN)
    while uncovered:
        seeds = [p for p in order if p in uncovered][:24]
        best = max((candidate(p) for p in seeds), key=lambda c: c[1])     # (max keeps the first of equal gains)
        take(best[0])
    return rows


# -- the table: sixteen levels, the seed, the graph.  Regenerate the levels with generate(); the seeds are the result of first_clear_seed().
ROWS = (
    ('records_d8', 'fp32', 'taps_off', 'L2', 'norm_none', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'node', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 5, 'parity'),
    ('records_d8', 'bf16', 'taps_on', 'L1', 'layer', 'linear', 'pf_on', 'pa_on', 'pe_on', 'fe3', 'readout_mean', 'bce', 'hid16_relu', 'mask_on', 'flat_off', 'fwd_bwd', 1, 'parity'),
    ('records_d4', 'fp32', 'taps_on', 'L3', 'layer_skip', 'bias', 'pf_0', 'pa_on', 'pe_keep_self', 'fe8', 'readout_sum', 'mse', 'hid5_lrelu', 'mask_off', 'flat_off', 'phases', 58, 'parity'),
    ('msg_rows_d16', 'bf16', 'taps_off', 'L3', 'batch', 'both', 'pf_on', 'pa_0', 'pe_shared', 'fe8', 'readout_max', 'softmax', 'hid16_relu', 'mask_on', 'flat_off', 'replay', 10, 'parity'),
    ('hd16', 'bf16', 'taps_on', 'L2', 'batch_skip', 'res_none', 'pf_on', 'pa_on', 'pe_0', 'fe0', 'pair_mul', 'mse', 'hid5_lrelu', 'mask_on', 'flat_off', 'replay', 0, 'parity'),
    ('generic', 'fp32', 'taps_off', 'L1', 'batch_skip', 'linear', 'pf_0', 'pa_0', 'pe_on', 'fe3', 'pair_add', 'mse', 'hid_off', 'mask_off', 'flat_off', 'fwd_bwd', 0, 'parity'),
    ('hd128_generic', 'fp32', 'taps_off', 'L2', 'layer', 'bias', 'pf_on', 'pa_0', 'pe_keep_self', 'fe0', 'readout_mean', 'bce', 'hid_off', 'mask_off', 'flat_off', 'phases', 0, 'parity'),
    ('hd128_generic', 'fp32', 'taps_on', 'L3', 'norm_none', 'both', 'pf_0', 'pa_on', 'pe_shared', 'fe3', 'pair_mul', 'bce', 'hid_off', 'mask_on', 'flat_off', 'step', 1, 'parity'),
    ('msg_rows_d16', 'fp32', 'taps_on', 'L1', 'batch', 'res_none', 'pf_0', 'pa_on', 'pe_keep_self', 'fe3', 'readout_max', 'softmax', 'hid5_lrelu', 'mask_off', 'flat_off', 'fwd_bwd', 4, 'parity'),
    ('records_d4', 'bf16', 'taps_off', 'L2', 'layer_skip', 'linear', 'pf_on', 'pa_0', 'pe_shared', 'fe0', 'readout_sum', 'softmax', 'hid16_relu', 'mask_off', 'flat_off', 'step', 1, 'small'),
    ('hd16', 'fp32', 'taps_off', 'L1', 'norm_none', 'bias', 'pf_0', 'pa_0', 'pe_on', 'fe8', 'pair_mul', 'softmax', 'hid16_relu', 'mask_off', 'flat_off', 'phases', 0, 'parity'),
    ('generic', 'fp32', 'taps_on', 'L3', 'layer', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe8', 'readout_mean', 'bce', 'hid5_lrelu', 'mask_on', 'flat_off', 'replay', 1, 'parity'),
    ('generic', 'fp32', 'taps_off', 'L2', 'layer_skip', 'both', 'pf_on', 'pa_on', 'pe_on', 'fe0', 'node', 'bce', 'hid5_lrelu', 'mask_on', 'flat_off', 'fwd_bwd', 0, 'parity'),
    ('records_d4', 'bf16', 'taps_off', 'L1', 'norm_none', 'both', 'pf_0', 'pa_0', 'pe_0', 'fe3', 'readout_sum', 'bce', 'hid_off', 'mask_on', 'flat_off', 'replay', 0, 'parity'),
    ('records_d8', 'bf16', 'taps_off', 'L3', 'batch_skip', 'bias', 'pf_0', 'pa_0', 'pe_keep_self', 'fe8', 'node', 'mse', 'hid16_relu', 'mask_on', 'flat_off', 'step', 23, 'parity'),
    ('msg_rows_d16', 'fp32', 'taps_off', 'L2', 'norm_none', 'linear', 'pf_on', 'pa_0', 'pe_0', 'fe8', 'pair_add', 'bce', 'hid5_lrelu', 'mask_on', 'flat_off', 'phases', 4, 'parity'),
    ('hd16', 'fp32', 'taps_off', 'L3', 'batch', 'linear', 'pf_0', 'pa_0', 'pe_on', 'fe0', 'readout_max', 'bce', 'hid_off', 'mask_off', 'flat_off', 'step', 3, 'parity'),
    ('hd128_generic', 'fp32', 'taps_off', 'L1', 'layer_skip', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'pair_add', 'softmax', 'hid16_relu', 'mask_off', 'flat_off', 'replay', 0, 'parity'),
    ('generic', 'fp32', 'taps_off', 'L2', 'batch', 'bias', 'pf_0', 'pa_0', 'pe_0', 'fe3', 'readout_max', 'mse', 'hid16_relu', 'mask_off', 'flat_off', 'phases', 5, 'parity'),
    ('hd16', 'fp32', 'taps_off', 'L1', 'layer', 'both', 'pf_0', 'pa_0', 'pe_shared', 'fe3', 'node', 'mse', 'hid5_lrelu', 'mask_off', 'flat_off', 'step', 0, 'parity'),
    ('msg_rows_d16', 'fp32', 'taps_off', 'L2', 'batch_skip', 'bias', 'pf_0', 'pa_0', 'pe_shared', 'fe0', 'readout_mean', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 5, 'parity'),
    ('hd128_generic', 'fp32', 'taps_off', 'L2', 'batch', 'res_none', 'pf_0', 'pa_0', 'pe_on', 'fe8', 'readout_sum', 'mse', 'hid_off', 'mask_off', 'flat_off', 'fwd_bwd', 3, 'parity'),
    ('records_d8', 'bf16', 'taps_on', 'L3', 'batch', 'both', 'pf_0', 'pa_on', 'pe_keep_self', 'fe0', 'pair_add', 'softmax', 'hid5_lrelu', 'mask_off', 'flat_off', 'phases', 12, 'parity'),
    ('records_d8', 'fp32', 'taps_off', 'L2', 'layer_skip', 'linear', 'pf_0', 'pa_0', 'pe_keep_self', 'fe3', 'pair_mul', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'replay', 6, 'parity'),
    ('records_d4', 'fp32', 'taps_off', 'L2', 'layer', 'res_none', 'pf_0', 'pa_0', 'pe_shared', 'fe0', 'pair_add', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'fwd_bwd', 10, 'parity'),
    ('hd128_generic', 'fp32', 'taps_off', 'L2', 'batch_skip', 'linear', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'node', 'bce', 'hid5_lrelu', 'mask_off', 'flat_off', 'phases', 2, 'parity'),
    ('hd16', 'fp32', 'taps_off', 'L2', 'norm_none', 'res_none', 'pf_0', 'pa_0', 'pe_keep_self', 'fe0', 'readout_mean', 'mse', 'hid_off', 'mask_off', 'flat_off', 'fwd_bwd', 0, 'parity'),
    ('records_d4', 'fp32', 'taps_on', 'L2', 'batch', 'res_none', 'pf_0', 'pa_0', 'pe_on', 'fe0', 'node', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'replay', 8, 'parity'),
    ('msg_rows_d16', 'fp32', 'taps_off', 'L2', 'layer', 'res_none', 'pf_0', 'pa_0', 'pe_on', 'fe0', 'readout_sum', 'mse', 'hid_off', 'mask_off', 'flat_off', 'phases', 9, 'parity'),
    ('records_d8', 'fp32', 'taps_off', 'L2', 'norm_none', 'res_none', 'pf_0', 'pa_0', 'pe_shared', 'fe0', 'node', 'softmax', 'hid_off', 'mask_off', 'flat_on', 'phases', 0, 'parity'),
    ('generic', 'fp32', 'taps_on', 'L1', 'norm_none', 'linear', 'pf_on', 'pa_on', 'pe_keep_self', 'fe3', 'node', 'softmax', 'hid_off', 'mask_on', 'flat_on', 'step', 0, 'parity'),
    ('msg_rows_d16', 'bf16', 'taps_off', 'L3', 'norm_none', 'bias', 'pf_0', 'pa_0', 'pe_0', 'fe8', 'node', 'softmax', 'hid_off', 'mask_off', 'flat_on', 'fwd_bwd', 3, 'parity'),
    ('records_d4', 'fp32', 'taps_off', 'L2', 'batch_skip', 'both', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_mean', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 5, 'parity'),
    ('hd16', 'fp32', 'taps_off', 'L2', 'layer_skip', 'bias', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'pair_add', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 1, 'parity'),
    ('generic', 'fp32', 'taps_off', 'L2', 'layer', 'res_none', 'pf_0', 'pa_0', 'pe_shared', 'fe0', 'pair_mul', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'fwd_bwd', 0, 'parity'),
    ('records_d4', 'fp32', 'taps_off', 'L2', 'norm_none', 'both', 'pf_0', 'pa_0', 'pe_on', 'fe0', 'node', 'softmax', 'hid_off', 'mask_off', 'flat_on', 'replay', 1, 'parity'),
    ('records_d8', 'fp32', 'taps_off', 'L2', 'norm_none', 'bias', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_max', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'replay', 11, 'parity'),
    ('msg_rows_d16', 'fp32', 'taps_off', 'L2', 'layer_skip', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_mean', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 14, 'parity'),
    ('records_d8', 'fp32', 'taps_off', 'L2', 'batch_skip', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_sum', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 160, 'parity'),
    ('records_d4', 'fp32', 'taps_off', 'L2', 'layer', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_max', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 9, 'parity'),
    ('records_d4', 'fp32', 'taps_off', 'L2', 'batch', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'pair_mul', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 5, 'parity'),
    ('hd128_generic', 'fp32', 'taps_off', 'L2', 'layer_skip', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_max', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 3, 'parity'),
    ('msg_rows_d16', 'fp32', 'taps_off', 'L2', 'norm_none', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'pair_mul', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 3, 'parity'),
    ('hd16', 'fp32', 'taps_off', 'L2', 'norm_none', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_sum', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 0, 'parity'),
    ('generic', 'fp32', 'taps_off', 'L2', 'norm_none', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_sum', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 1, 'parity'),
    ('hd16', 'fp32', 'taps_off', 'L2', 'norm_none', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'node', 'softmax', 'hid_off', 'mask_off', 'flat_on', 'step', 0, 'parity'),
    ('hd128_generic', 'fp32', 'taps_off', 'L2', 'norm_none', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'node', 'softmax', 'hid_off', 'mask_off', 'flat_on', 'step', 0, 'parity'),
    ('records_d8', 'fp32', 'taps_off', 'L2', 'batch', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_mean', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 1, 'parity'),
    ('records_d8', 'fp32', 'taps_off', 'L2', 'batch_skip', 'res_none', 'pf_0', 'pa_0', 'pe_0', 'fe0', 'readout_max', 'softmax', 'hid_off', 'mask_off', 'flat_off', 'step', 1, 'parity'),
)


def levels_of(row):
    return dict(zip(NAMES, row[:len(NAMES)]))


def row_id(i):
    return f"row{i:02d}"


# -- the builder
def _dims(family, layers):
    """A family's first (H, D), then its second for every later layer."""
    _, heads, outdims, _ = next(f for f in FC.FAMILIES if f[0] == family)
    n = int(layers[1])
    return [heads[0]] + [heads[1]] * (n - 1), [outdims[0]] + [outdims[1]] * (n - 1)


def _self_loops(g):
    """make_graph(self_loops=True)'s construction on a finished graph: the first edge of every non-empty row becomes the row's self-loop."""
    rp, ci = g["row_ptr"], g["col_idx"].copy()
    ne = np.diff(rp) > 0
    ci[rp[:-1][ne]] = np.arange(g["n"], dtype=np.int32)[ne]
    return dict(g, col_idx=ci)


def graph_of(lv, which):
    heads, outdims = _dims(lv["family"], lv["layers"])
    if max(h * d for h, d in zip(heads, outdims)) >= 128:
        g = FC.wide_graph()
    elif which == "parity":
        g = FC.parity_graph()
    else:
        assert which == "small"
        g = FC.host_graph(5)
    return _self_loops(g) if lv["dropedge"] == "pe_keep_self" else g


def graph_ptr_for(n):
    """readout_ref.GRAPH_PTR on 150 nodes; the same shape on another count: an empty graph, two single-node graphs, two larger ones."""
    return list(RR.GRAPH_PTR) if n == RR.GRAPH_PTR[-1] else [0, 0, 1, n // 3, n // 3 + 1, n]


def steps_of(lv):
    """Steps the row's context takes before it is compared: a captured step graph is compared at its second replay (warm-up, capture +
    launch, replay)."""
    return 3 if lv["path"] == "replay" else 1


@functools.lru_cache(maxsize=None)
def _static(levels, which):
    """Everything of a row that does not depend on the parameter seed."""
    import __graft_entry__ as entry
    pkg, orc = entry.load_package(), entry.load_oracle()
    lv = dict(zip(NAMES, levels))
    g = graph_of(lv, which)
    loss = lv["loss"]
    if loss == "bce":                                    # C = 1: the link-prediction head
        g = dict(g, c=1, labels=np.zeros(g["n"], np.int32))
    heads, outdims = _dims(lv["family"], lv["layers"])
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    head = lv["head"]
    kind = "readout" if head.startswith("readout") else head
    pool = head.split("_")[1] if kind == "readout" else "mean"
    graph_ptr = graph_ptr_for(g["n"]) if kind == "readout" else None
    u, v = PR.pair_list(g["n"]) if kind.startswith("pair") else (None, None)
    rows = len(u) if u is not None else len(graph_ptr) - 1 if graph_ptr is not None else g["n"]
    if loss == "softmax":
        sup = g["labels"] if kind == "node" else PR.pair_labels(rows, g["c"])
    elif loss == "bce":
        sup = (np.random.default_rng(41).random((rows, 1)) > 0.5).astype(np.float32)
    else:
        sup = LR.targets_for(pkg, "mse", rows, g["c"])   # NaN holes
    mask = LR.row_mask(rows) if lv["mask"] == "mask_on" else None
    dh, act = {"hid_off": (0, "relu"), "hid16_relu": (16, "relu"), "hid5_lrelu": (5, "lrelu")}[lv["hidden"]]
    W1, b1, Wo_h = HM.head_values(outdims[-1], dh, g["c"]) if dh else (None, None, None)
    fe = int(lv["edge_feat"][2:])
    ea = EF.edge_attrs(g, fe) if fe else None
    pf = REG["pf"] if lv["feat_drop"] == "pf_on" else 0.0
    pa = REG["pa"] if lv["attn_drop"] == "pa_on" else 0.0
    pe = REG["pe"] if lv["dropedge"] != "pe_0" else 0.0
    norm = lv["norm"]
    return dict(lv=lv, g=g, heads=heads, outdims=outdims, cfg=cfg, kind=kind, pool=pool, graph_ptr=graph_ptr, u=u, v=v, rows=rows, loss=loss,
                sup=sup, mask=mask, dh=dh, act=act, W1=W1, b1=b1, Wo_h=Wo_h, fe=fe, ea=ea, pf=pf, pa=pa, pe=pe,
                keep_self=lv["dropedge"] == "pe_keep_self", shared=lv["dropedge"] == "pe_shared", normed=norm != "norm_none",
                bn=norm.startswith("batch"), skip_last=norm.endswith("_skip"), lin=lv["residual"] in ("linear", "both"),
                bias=lv["residual"] in ("bias", "both"), bf16=lv["dtype"] == "bf16", flat=lv["flat"] == "flat_on",
                keep_taps=lv["keep_taps"] == "taps_on", steps=steps_of(lv))


def masks(st, step):
    """(keeps, attn, feat) of training step `step` (the counter starts at 0 and advances once per training forward); None where off."""
    cfg, g, seed = st["cfg"], st["g"], REG["seed"]
    L = range(cfg.L)
    keeps = [E.edge_keep(seed, step, l, g["row_ptr"], g["col_idx"], st["pe"], keep_self=st["keep_self"], shared=st["shared"])
             for l in L] if st["pe"] else None
    attn = [R.attn_factor(seed, step, l, g["row_ptr"], cfg.heads[l], st["pa"]) for l in L] if st["pa"] else None
    feat = [R.feat_factor(seed, step, l, g["n"], cfg.in_dims[l], st["pf"]) for l in L] if st["pf"] else None
    return keeps, attn, feat


def params(st, seed):
    """The parameter groups of the row at Xavier seed `seed`: (W, a, Wo) and the dict of the others (None where the row lacks one)."""
    import __graft_entry__ as entry
    orc = entry.load_oracle()
    cfg = st["cfg"]
    P = orc.xavier_params(cfg, seed)
    Wres, b = SR.xavier_wres(cfg, seed)
    gamma, beta = SR.ln_params(cfg, seed) if st["normed"] else (None, None)
    inp = dict(Wres=Wres if st["lin"] else None, b=b if st["bias"] else None, gamma=gamma, beta=beta,
               ea=st["ea"], We=SR.xavier_we(cfg, st["fe"], seed) if st["fe"] else None)
    return P, inp


def model(st, P, inp, training=True, running=None, step=1):
    """tests/step_ref.py::forward of the row (before backward).  training=False: eval mode on `running`, no masks."""
    g = st["g"]
    head = HD.head(st["kind"], st["loss"], st["sup"], st["mask"], graph_ptr=st["graph_ptr"], u=st["u"], v=st["v"], pool_mode=st["pool"],
                   Wo=st["Wo_h"] if st["dh"] else P[2], W1=st["W1"], b1=st["b1"], act_name=st["act"], detach_max=False, smooth_bce=True)
    keeps, attn, feat = masks(st, step) if training else (None, None, None)
    return SR.forward(st["cfg"], g["row_ptr"], g["col_idx"], None, g["x"], P[0], P[1], None, **inp, eps=FC.EPS, skip_last=st["skip_last"],
                      keeps=keeps, attn=attn, feat=feat, bf16_pl=st["bf16"], flat_lrelu_index=st["flat"], bn=st["bn"], training=training,
                      running=running, momentum=BC.MOMENTUM, head=head)


def model_steps(st, P, inp):
    """The model of the step the row is compared at: step steps_of(row), and with batch normalisation the running statistics of all the
    steps before it (the parameters stand still; the masks of every step are its own)."""
    running = None
    for k in range(1, st["steps"]):
        if st["bn"]:
            r = model(st, P, inp, running=running, step=k)
            running = (r["running_mean"], r["running_var"])
    return model(st, P, inp, running=running, step=st["steps"])


def clear(st, ref):
    """The row's clearness conditions on the model's outputs: every non-zero |s| > 1e-5; |h_pre| > 1e-5, or |v| > 1e-4 with a norm; with
    the hidden layer |A + b1| > A_MIN; softmax rows that train above Y_MIN; for the MAX readout a clear winner in every (graph, column)."""
    if not (FC.CLEAR_V if st["normed"] else FC.CLEAR_HPRE)(ref):
        return False
    if st["dh"] and not float(np.abs(ref["pre"]).min()) > HM.A_MIN:
        return False
    if st["loss"] == "softmax":
        keep = np.ones(st["rows"], bool) if st["mask"] is None else np.asarray(st["mask"], bool)
        if not float(ref["y"][np.arange(st["rows"]), np.asarray(st["sup"])][keep].min()) > HM.Y_MIN:
            return False
    if st["kind"] == "readout" and st["pool"] == "max":
        x = ref["hout"][-1].detach().numpy()
        if not RR.pool_gap(x, st["graph_ptr"], "max") > RR.GAP * np.abs(x).max():
            return False
    return True


def seed_is_clear(levels, which, seed):
    st = _static(tuple(levels), which)
    P, inp = params(st, seed)
    return clear(st, model_steps(st, P, inp))


def first_clear_seed(levels, which, below=BC.SEEDS):
    """The first seed below `below` whose model is clear, or None."""
    return next((s for s in range(below) if seed_is_clear(levels, which, s)), None)


@functools.lru_cache(maxsize=None)
def case(i):
    """Everything row i runs on: _static's dict with P, inp and ref — the fp64 model of the compared step AFTER loss.backward() — and
    eval_ref, the eval-mode model on the running statistics that step left (cached: one evaluation per row and process)."""
    row = ROWS[i]
    st = dict(_static(tuple(row[:len(NAMES)]), row[-1]))
    P, inp = params(st, row[-2])
    ref = model_steps(st, P, inp)
    ref["loss"].backward()
    for k in ("W1", "b1"):
        ref.setdefault(k, None)                          # a row without the hidden layer: the groups are absent
    running = (ref["running_mean"], ref["running_var"]) if st["bn"] else None
    st.update(index=i, seed=row[-2], which=row[-1], P=P, inp=inp, ref=ref, eval_ref=model(st, P, inp, training=False, running=running))
    return st


def make_ctx(pkg, st, P=None, inp=None, cls=None, **kw):
    """A context of the row, every parameter group it has set, gradients zeroed.  The gat_set_* calls in the header's order: the
    layout calls (normaliser, edge_dim, residual, hidden layer) before anything sizes the buffers, the loss before the supervision,
    readout / pairs between the graph and the supervision, the regularisers and the mask last.  cls: a subclass of GatContext to build
    (the refusal tests trace the calls with one); **kw goes to GatContext."""
    A = pkg.abi
    g = st["g"]
    P = st["P"] if P is None else P
    inp = st["inp"] if inp is None else inp
    ctx = (cls or pkg.GatContext)(st["heads"], st["outdims"], g["f"], g["c"], **dict(dict(dtype="bf16" if st["bf16"] else "f32", keep_taps=st["keep_taps"],
                                                                                 flat_lrelu_index=st["flat"]), **kw))
    if st["normed"] and st["bn"]:
        ctx.set_batch_norm(skip_last=st["skip_last"], eps=FC.EPS, momentum=BC.MOMENTUM)
    elif st["normed"]:
        ctx.set_norm(skip_last=st["skip_last"], eps=FC.EPS)
    if st["fe"]:
        ctx.set_edge_dim(st["fe"])
    if st["lin"] or st["bias"]:
        ctx.set_residual(linear=st["lin"], bias=st["bias"])
    if st["loss"] != "softmax":
        ctx.set_loss(st["loss"])
    if st["dh"]:
        ctx.set_head_hidden(st["dh"], st["act"])
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    if st["kind"] == "readout":
        ctx.set_readout(st["pool"], graph_ptr=st["graph_ptr"])
    elif st["kind"].startswith("pair"):
        ctx.set_pairs(st["kind"][5:], st["u"], st["v"])
    if st["loss"] == "softmax":
        ctx.set_labels(st["sup"])
    else:
        ctx.set_targets(st["sup"])
    if st["fe"]:
        ctx.set_edge_features(st["ea"])
    for grp, name in ((A.PARAM_WRES, "Wres"), (A.PARAM_B, "b"), (A.PARAM_NORM_G, "gamma"), (A.PARAM_NORM_B, "beta"), (A.PARAM_WE, "We")):
        if inp.get(name) is not None:
            ctx.params_set(grp, inp[name])
    ctx.params_set(A.PARAM_W, P[0]); ctx.params_set(A.PARAM_A, P[1]); ctx.params_set(A.PARAM_WO, st["Wo_h"] if st["dh"] else P[2])
    if st["dh"]:
        ctx.params_set(A.PARAM_HEAD_W, st["W1"]); ctx.params_set(A.PARAM_HEAD_B, st["b1"])
    if st["pf"] or st["pa"] or st["pe"]:
        ctx.set_dropout(st["pf"], st["pa"], seed=REG["seed"], first_step=0)
        ctx.set_dropedge(st["pe"], keep_self=st["keep_self"], shared_layers=st["shared"])
    if st["mask"] is not None:
        ctx.set_train_mask(st["mask"])
    ctx.zero_grad()
    return ctx


def fused_eligible(lv):
    """gat_abi_step.hip::fused_last restated on a row's levels: what GAT_FUSE_LAST=1 fuses (gat_step only)."""
    return (lv["family"] == "records_d8" and lv["dtype"] == "fp32" and lv["keep_taps"] == "taps_off" and lv["norm"] == "norm_none"
            and lv["residual"] == "res_none" and lv["feat_drop"] == "pf_0" and lv["attn_drop"] == "pa_0" and lv["dropedge"] == "pe_0"
            and lv["edge_feat"] == "fe0" and lv["head"] == "node" and lv["loss"] == "softmax" and lv["hidden"] == "hid_off"
            and lv["flat"] == "flat_off")


# -- the kernel picks: one child process per profile (the switches are read once per process)
PROFILES = {
    "default": {},
    "records_groups": {"GAT_PULL_LAST": "1", "GAT_PULL_GROUPS": "1", "GAT_GPL_HEAVY": "16", "GAT_SEG_EDGES": "16"},
    "slot_runs": {"GAT_PULL_RUNS": "1", "GAT_PULL_LAST": "1", "GAT_SEG_EDGES": "16"},
    "fuse_last": {"GAT_FUSE_LAST": "1", "GAT_PULL_LAST": "1"},
}


# -- a row on the GPU (tests/test_feature_pairs.py and its child processes)
GENERIC = ("generic", "hd128_generic")                   # layer 0 scatters gPL with float atomics: grad_W is order-dependent at round-off


def take_steps(ctx, st, path):
    """The row's steps on `path`, gradients zeroed before each -> (loss, correct) of the last.  "replay": gat_step under gat_step_graph —
    eager warm-up, capture + launch, replay; "phases": the order of tests/test_batchnorm.py::test_paths_agree."""
    L = st["cfg"].L
    if path == "replay":
        ctx.step_graph(True)
    for _ in range(st["steps"]):
        ctx.zero_grad()
        if path in ("step", "replay"):
            out = ctx.step()
        elif path == "fwd_bwd":
            out = ctx.forward()
            ctx.backward()
        else:
            assert path == "phases"
            for l in range(L):
                ctx.layer_project(l); ctx.layer_forward_edges(l)
            out = ctx.head_forward()
            ctx.head_backward()
            for l in range(L - 1, -1, -1):
                ctx.layer_backward_edges(l); ctx.layer_backward_dense(l)
    if path == "replay":
        assert ctx.step_graph_state() == 2
    return out


def compare(pkg, ctx, st, loss):
    """The context after the row's steps against the fp64 model, at 1e-4 of max-abs (1e-2 with bf16 storage), every error recorded: loss
    per row, h_pre / hout / G of every layer, the ten gradient groups (one the row lacks is empty on the device), the statistics of a
    batch-norm row, the pooled / pair / hidden rows, with keep_taps alpha and score; the exact zeros of skip_last and of the mask."""
    import parity
    A = pkg.abi
    cfg, ref, g = st["cfg"], st["ref"], st["g"]
    tol = 1e-2 if st["bf16"] else 1e-4
    L = cfg.L
    lo = SR.ln_offsets(cfg)
    dead = st["normed"] and st["skip_last"] and L == 1       # the only layer is the one left un-normalised: gamma / beta are never read
    groups = [k for k in SR.GROUPS if k != "b" and not (dead and k in ("gamma", "beta"))]
    FC.compare(pkg, ctx, dict(g, n=HM.loss_rows(st)), cfg, ref, loss, tol, ["hpre", "hout", "G"], groups)
    got = FC.grads(pkg, ctx, ["b"])[0]                       # grad_b under batch normalisation vanishes: bn_cases.compare says what it is held to
    if ref["b"] is None:
        assert got.size == 0
    else:
        want = ref["b"].grad.numpy()
        terms = max(float(ref["hpre"][l].grad.abs().reshape(g["n"], -1).sum(0).max()) for l in range(L))
        vanishing = st["bn"] and float(np.abs(want).max()) <= 1e-9 * terms
        assert got.shape == want.shape and (vanishing or np.abs(want).max() > 0)
        parity.check_rel("grad b", got, want, tol, floor=terms if vanishing else 1e-12, vanishing=vanishing)
    if st["normed"] and st["skip_last"]:
        for k in (A.PARAM_NORM_G, A.PARAM_NORM_B):
            gk = ctx.grads_get(k)
            assert gk.size == lo[-1] and (gk[lo[L - 1]:] == 0).all(), "skip_last: the skipped layer's gamma / beta gradients are exactly 0"
    if st["bn"]:
        if not dead:
            BC.compare_stats(pkg, ctx, ref, tol)
        if st["skip_last"]:
            for which, fresh in enumerate((0.0, 1.0, 0.0, 0.0)):
                assert (ctx.batch_norm_stats(which)[lo[L - 1]:] == fresh).all()
    if st["kind"] == "readout":
        parity.check_rel("pooled", ctx.tap(A.TAP_POOLED, L - 1), ref["xin"].detach().numpy(), tol)
    elif st["kind"].startswith("pair"):
        parity.check_rel("paired", ctx.tap(A.TAP_PAIRED, L - 1), ref["xin"].detach().numpy(), tol)
    if st["dh"]:
        parity.check_rel("Z1", ctx.tap(A.TAP_HEAD_HIDDEN, L - 1), ref["z1"].detach().numpy(), tol)
    if st["keep_taps"]:
        keeps = masks(st, st["steps"])[0]
        for l in range(L):
            keep = np.ones(len(g["col_idx"]), bool) if keeps is None else keeps[l]
            alpha = ctx.tap(A.TAP_ALPHA, l)
            assert (alpha[:, ~keep] == 0).all()
            parity.check_rel(f"alpha[{l}]", alpha, ref["alpha"][l], tol)
            parity.check_rel(f"score[{l}]", ctx.tap(A.TAP_SCORE, l)[:, keep], ref["score"][l][:, keep], tol)
    if st["mask"] is not None and st["kind"] == "node" and not st["normed"]:
        assert not ctx.tap(A.TAP_G, L - 1)[~st["mask"]].any()    # dz is exactly 0 outside the training mask (tests/head_cases.py)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare_with_step(pkg, ctx, st, out):
    """A second context of the row on plain gat_step: loss, correct, every gradient group and the statistics bitwise the row's path
    (generic families: grad_W at 1e-5 of max-abs, tests/test_batchnorm.py::test_paths_agree)."""
    with make_ctx(pkg, st) as s:
        assert take_steps(s, st, "step") == out, ("loss / correct differ from gat_step", out)
        for k, x, y in zip(SR.GROUPS, FC.grads(pkg, ctx, SR.GROUPS), FC.grads(pkg, s, SR.GROUPS)):
            if k == "W" and st["lv"]["family"] in GENERIC:
                assert np.abs(x - y).max() <= 1e-5 * np.abs(y).max(), k
            else:
                assert np.array_equal(_bits(x), _bits(y)), f"grad {k} differs from gat_step"
        if st["bn"]:
            for i, (x, y) in enumerate(zip(BC.all_stats(ctx), BC.all_stats(s))):
                assert np.array_equal(_bits(x), _bits(y)), f"{BC.STATS[i]} differs from gat_step"


def compare_eval(pkg, ctx, st):
    """gat_set_training(0) + gat_forward against the eval-mode model on the statistics the step left: no dropout, no DropEdge."""
    import parity
    A = pkg.abi
    tol = 1e-2 if st["bf16"] else 1e-4
    ctx.set_training(False)
    loss, _ = ctx.forward()
    ev, n = st["eval_ref"], HM.loss_rows(st)
    parity.check_abs("eval loss/N", loss / n, ev["loss"].item() / n, tol)
    for l in range(st["cfg"].L):
        w = ev["hout"][l].detach().numpy()
        parity.check_rel(f"eval hout[{l}]", ctx.tap(A.TAP_HOUT, l).reshape(w.shape), w, tol)


def run_row(pkg, i):
    """Row i: one context on the row's step path against the model, a second on gat_step against the first, then eval mode.  The row
    GAT_FUSE_LAST=1 fuses runs with collect_timing, and the fused kernel's launch count says whether it ran: it must exactly when the
    switch is set."""
    A = pkg.abi
    st = case(i)
    fusable = fused_eligible(st["lv"]) and st["lv"]["path"] == "step"
    with make_ctx(pkg, st, collect_timing=fusable) as ctx:
        if fusable:
            ctx.kernel_stats_reset()
        out = take_steps(ctx, st, st["lv"]["path"])
        if fusable:
            ran = ctx.kernel_stats()[ctx.lib.gat_kernel_name(A.K_EDGE_FUSED).decode()][0] > 0
            assert ran == ("GAT_FUSE_LAST=1" in A.switches().split()), ("the fused last layer", ran, A.switches())
        compare(pkg, ctx, st, out[0])
        compare_with_step(pkg, ctx, st, out)
        compare_eval(pkg, ctx, st)


def run_table(pkg, profile):
    """Every row in this process -> (rows that passed, the ids of those that failed).  An assertion or a refusal of the library fails the
    row and the table goes on; anything else — a HIP error among them — ends the process."""
    import parity
    A = pkg.abi
    ok, failed = 0, []
    for i in range(len(ROWS)):
        parity.set_test(f"tests/test_feature_pairs.py::test_table_under_the_profile[{profile}] {row_id(i)}")
        try:
            run_row(pkg, i)
            ok += 1
        except (AssertionError, A.GatError) as e:
            if isinstance(e, A.GatError) and e.code not in (10001, 10002, 10004):
                raise
            failed.append(row_id(i))
            print("FAILED", row_id(i), " ".join(ROWS[i][:len(NAMES)]), "|", type(e).__name__, str(e)[:400], flush=True)
    return ok, failed
