"""The feature forms of the edge kernels under the picks the FULL-SIZE shapes take (tests/test_full_size_picks.py and its _cpu twin).

Every graph of the suite has a few thousand edges, so build_worklist (csrc/gat_abi_data.hip) cuts its rows into segments of 16: the
group-per-row kernels only ever walk items of 16 edges or fewer and only ever close such rows in their epilogue; the full-size shapes
walk rows of up to 256 edges as one item.  Here: the switch settings that reproduce the defaults of four BASELINE shapes on a small
graph (PROFILES), a graph with rows of the lengths those settings treat differently (long_rows_graph), the case table (CASES) and the
worker that runs it in a process of one profile against the fp64 model of tests/step_ref.py.
A plain module, like tests/feature_cases.py."""
import numpy as np

import edge_feat_ref as EF
import feature_cases as FC
import parity
from feature_cases import FORMS, REG

# -- the rules, restated (tests/test_full_size_picks_cpu.py derives PROFILES from them and the BASELINE shapes)
SEG_DEFAULT = 256


def seg_edges(n_edges):
    """build_worklist: the segment length by graph size."""
    return 16 if n_edges < (512 << 10) else 32 if n_edges < (4 << 20) else 64 if n_edges < (16 << 20) else SEG_DEFAULT


def short_lists_take_runs(n_slots, n_table):
    """gat_internal.h: the slot-parallel pull is the default on short lists, and enough of them."""
    return n_slots < 8 * n_table and n_slots >= (512 << 10)


def node_records(n_rows, hd, runs, bf16):
    """plan_backward_edges: the last layer's pull rebuilds g from node records where the g rows are large (fp32 only)."""
    return not bf16 and n_rows * hd * 4 > ((64 if runs else 128) << 20)


# name -> environment.  The switches are CHOICE switches, read once per process: one process per profile.
PROFILES = {
    "products": {"GAT_SEG_EDGES": "256", "GAT_PULL_LAST": "1"},
    "arxiv": {"GAT_SEG_EDGES": "32", "GAT_PULL_RUNS": "1", "GAT_PULL_LAST": "0"},
    "products_p8": {"GAT_SEG_EDGES": "64", "GAT_PULL_RUNS": "1", "GAT_PULL_LAST": "1"},
    "config5": {"GAT_SEG_EDGES": "256", "GAT_PULL_LAST": "0"},
}
# name -> (n_rows, n_table, n_edges, H*D of the last layer, bf16 storage, the text of its BASELINE.json entry)
PROFILE_SHAPES = {
    "products": (2_450_000, 2_450_000, 61_900_000, 64, False, "2.45M / 61.9M"),
    "arxiv": (169_000, 169_000, 1_170_000, 64, False, "169k / 1.17M"),
    # a destination-range shard: an eighth of the rows and edges, the table stays the whole graph's
    "products_p8": (2_450_000 // 8, 2_450_000, 61_900_000 // 8, 64, False, "2.45M / 61.9M"),
    "config5": (10_000_000, 10_000_000, 250_000_000, 32, True, "10M nodes / 250M edges"),
}


def profile_env(n_rows, n_table, n_edges, hd, bf16):
    """The environment that makes a small graph take the picks this shape takes by default."""
    runs = short_lists_take_runs(n_edges, n_table)
    env = {"GAT_SEG_EDGES": str(seg_edges(n_edges))}
    if runs:                                     # off is the small graph's own default: nothing to set
        env["GAT_PULL_RUNS"] = "1"
    env["GAT_PULL_LAST"] = "1" if node_records(n_rows, hd, runs, bf16) else "0"
    return env


# -- the graph
# row -> in-edges.  The masks are keyed by (row, position): rows 14 and 39 are where REG's DropEdge mask drops a whole step of four edges
# between positions 16 and 31 on BOTH layers, so rows that stay one item at segments of 32 carry such a step too
LONG_ROWS = {5: 33, 9: 256, 14: 32, 20: 17, 27: 64, 33: 257, 39: 31, 50: 16, 58: 65, 66: 15, 75: 63}
EMPTY_ROWS = (3, 95)
HUB = 11


def long_rows_graph():
    """96 nodes, F = 24, C = 5: rows of 15, 16, 17, 31, 32, 33, 63, 64, 65, 256 and 257 in-edges at scattered row numbers and in no
    order of length (the groups of a wave walk unequal rows), two empty rows (one the last), every other row 1 to 5 in-edges; 30 % of
    all edges come from node 11, whose source list then has more than 256 slots and crosses several 64-slot runs."""
    rng = np.random.default_rng(7)
    n, F, C = 96, 24, 5
    deg = rng.integers(1, 6, n)
    for r, d in LONG_ROWS.items():
        deg[r] = d
    deg[list(EMPTY_ROWS)] = 0
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    src = rng.integers(0, n, int(rp[-1]))
    src[rng.random(len(src)) < 0.3] = HUB
    ci = np.concatenate([np.sort(src[rp[r]:rp[r + 1]]) for r in range(n)]).astype(np.int32)
    x = rng.standard_normal((n, F)).astype(np.float32)
    lab = rng.integers(0, C, n).astype(np.int32)
    return dict(row_ptr=rp, col_idx=ci, x=x, labels=lab, n=n, f=F, c=C)


def worklist(row_ptr, seg):
    """build_worklist's items [(row, begin, end)] in its order: the segments of the split rows, then every other row as one item, longest
    first with the row order kept inside a length (one sort window: fewer than 4096 rows).  -> (split, whole)"""
    rp = np.asarray(row_ptr, np.int64)
    split, whole = [], []
    for r in range(len(rp) - 1):
        b, e = int(rp[r]), int(rp[r + 1])
        if e - b > seg:
            split += [(r, s, min(e, s + seg)) for s in range(b, e, seg)]
        else:
            whole.append((r, b, e))
    assert len(rp) - 1 <= 4096
    return split, sorted(whole, key=lambda it: it[1] - it[2])


# -- the cases
FE = 3
# (name, heads, outdims, storage)
MODELS = [(f"hd{hd}_d{d}", [hd // d] * 2, [d] * 2, dt)
          for hd, d, dt in [(64, 8, "fp32"), (64, 4, "fp32"), (64, 16, "fp32"), (32, 8, "fp32"), (8, 4, "fp32"), (64, 8, "bf16"), (32, 8, "bf16")]]
GENERIC = ("generic", [3, 2], [5, 8], "fp32")
PLAIN_FORMS = {"plain": (False, False, False), **FORMS}      # form -> (norm + residual, REG, keep_taps)
# (model name, heads, outdims, storage, form, edge_dim)
CASES = [(*m, form, 0) for m in MODELS + [GENERIC] for form in PLAIN_FORMS if form != "taps_res_norm_reg" or m[0] == "hd64_d8"]
CASES += [(*m, form, FE) for m in MODELS for form in ("plain", "res_norm_reg")]
TOL = {"fp32": 1e-4, "bf16": 1e-2}
TAPS = ["hpre", "hout", "G"]


def case_id(case):
    name, _, _, dt, form, fe = case
    return f"{name}-{dt}-{form}" + (f"-fe{fe}" if fe else "")


def case_config(orc, case, graph=None):
    """graph: (name, graph dict) instead of long_rows_graph (tests/trip_cases.py)."""
    g = long_rows_graph() if graph is None else graph[1]
    return g, orc.Config(case[1], case[2], g["f"], g["c"])


_REFS = {}


def reference(orc, case, graph=None):
    """(W, a, Wo), the other inputs, the fp64 model after its backward: once per model and graph (the keep_taps form shares res_norm_reg's).
    The seed search and its bounds are the ones of the parent tests (FC.pick_shape, EF.pick)."""
    name, heads, outdims, dt, form, fe = case
    norm, reg, _ = PLAIN_FORMS[form]
    key = (name, dt, norm, reg, fe, None if graph is None else graph[0])
    if key not in _REFS:
        g, cfg = case_config(orc, case, graph)
        if fe:
            out = EF.pick(FC, orc, cfg, g, fe, REG if reg else None, res_norm=norm, bf16=dt == "bf16")
        else:
            out = FC.pick_shape(orc, cfg, g, norm, REG if reg else None, dt == "bf16")
        out[-1]["loss"].backward()
        _REFS[key] = out
    return _REFS[key]


def run_case(pkg, orc, case, graph=None):
    """One context and one step of a case against its model, at the bar of the storage mode (graph: see case_config)."""
    name, heads, outdims, dt, form, fe = case
    norm, reg, taps = PLAIN_FORMS[form]
    A = pkg.abi
    g, cfg = case_config(orc, case, graph)
    P, inp, ref = reference(orc, case, graph)
    kw = {}
    if dt == "bf16":
        kw["dtype"] = "bf16"
    if taps:
        kw["keep_taps"] = True
    tol = TOL[dt]
    if fe:
        ctx = EF.make_ctx(pkg, g, heads, outdims, P, fe, **inp, reg=REG if reg else None, **kw)
    else:
        setters = FC.setters(FC.NORM_MODES[1], norm=True) if norm else {}
        ctx = FC.make_ctx(pkg, g, heads, outdims, P, **inp, **setters, reg=REG if reg else None, **kw)
    with ctx:
        loss, _ = ctx.step()
        if fe:
            EF.compare_all(pkg, ctx, g, cfg, ref, loss, tol)
        else:
            FC.compare(pkg, ctx, g, cfg, ref, loss, tol, taps=TAPS, groups=FC.GROUPS[:7])
        if taps:
            for l in range(cfg.L):
                want = ref["alpha"][l]
                assert np.abs(want).max() > 0
                got = ctx.tap(A.TAP_ALPHA, l)
                assert got.shape == want.shape
                parity.check_rel(f"alpha[{l}]", got, want, tol)
                keep = ctx.tap(A.TAP_EDGE_KEEP, l) != 0
                assert 0 < keep.sum() < keep.size
                assert np.array_equal(keep, want[0] != 0)        # the model's mask is the device's
                assert (got[:, ~keep] == 0).all()


def run_profile(pkg, orc, profile):
    """Every case in this process (whose environment is the profile's).  A failing comparison does not stop the others: it is printed
    with its profile, model, storage mode and form, and the achieved errors of all cases are written out.  -> (cases run, failures)"""
    failures = []
    for case in CASES:
        parity.set_test(f"full-size picks {profile}: {case_id(case)}")
        try:
            run_case(pkg, orc, case)
        except AssertionError as e:
            failures.append(f"{profile}: {case_id(case)}: {e}")
            print("FAILED", failures[-1])
    parity.flush()
    return len(CASES), failures
