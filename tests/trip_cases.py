"""The persistent kernels when a block walks MANY items (tests/test_grid_trips.py and its _cpu twin).

Several kernels size their grid as "what is resident at once" and let each block or wave loop over its items (`q += nwaves`,
`row += gridDim.x * rpb`).  On the graphs of the suite the resident count is far above the item count, so those loops run at most once
and nothing a wave carries from one trip into the next — prefetched indices, pending records, the running grad_a, dropout keys — is
ever compared with anything, except for the plain model at full size.  GAT_RESIDENT_CAP=<n> bounds every such grid: with
n = 1 a graph of a few hundred rows walks several trips per block, with n = 3 the blocks get unequal trip counts.

Here: the profiles (environment of one process each), the graphs on which trips happen and parameter seeds clear of the kinks still
exist, the case tables and the worker that runs the table of a profile.  No model and no comparison of its own: the edge forms go through
tests/pick_profiles.py (fp64 models of step_ref / edge_feat_ref), the heads through head_mlp_ref, pair_ref, loss_ref, head_cases and the
comparison functions of their tests, at those tests' bars.  A plain module, like tests/pick_profiles.py."""
import numpy as np

import feature_cases as FC
import head_cases as HC
import head_mlp_ref as HM
import loss_ref as LR
import pair_ref as PR
import parity
import pick_profiles as PP

# name -> environment.  The switches are read once per process: one process per profile.
PROFILES = {
    "cap1": {"GAT_RESIDENT_CAP": "1"},
    "cap3": {"GAT_RESIDENT_CAP": "3"},                     # several blocks, unequal trip counts
    "cap1_fused": {"GAT_RESIDENT_CAP": "1", "GAT_FUSE_LAST": "1"},
    "cap1_wave_rows": {"GAT_RESIDENT_CAP": "1", "GAT_ROWGROUP": "0", "GAT_GROUP_MSG": "0"},      # the wave-per-row backward kernels
}
# seconds a profile's process may take: the fp64 models and seed searches dominate (measured: the edge and head tables of cap1 / cap3 about
# 6 s side by side on four threads each, the other two under 3 s; the limits leave a loaded host a factor of 40)
TIMEOUT = {"cap1": 240, "cap3": 240, "cap1_fused": 120, "cap1_wave_rows": 120}

# -- the rules, restated (tests/test_grid_trips_cpu.py derives the trip counts from them)
SEG = 16                # build_worklist (gat_abi_data.hip:14): the segment length of a graph below 512 Ki edges
MAX_N = 4               # gat_edge_kernels.hip:1209  LPE = HD / N, G = 64 / LPE with N <= 4 channels per lane (stash_n, :2149)
WAVES = 4               # waves of a backward block: q = blockIdx.x * 4 + wave (:1236), nwaves = gridDim.x * 4
HEAD_TILE = 128         # head_blocks / head_bwd_blocks (gat_head.hip:667, :673): 128-row tiles
K_U = 4                 # gat_head_hidden.hip: kU rows per lane and trip


def group_items_max(hd):
    """G <= 256 / (H*D): the items a wave of the group-per-row backward holds side by side."""
    return 64 // (hd // MAX_N) if hd >= MAX_N else 64


def items_needed(hd):
    """Three full trips of the four waves of one block and a ragged fourth."""
    return 3 * WAVES * 256 // hd + 1


def edge_blocks(n_items, cap):
    """edge_backward_blocks (gat_edge_kernels.hip): min(ceil(n_items / 4), resident, kGaPartialRows) with resident = the cap."""
    return max(1, min((n_items + 3) // 4, cap))


def strided_trips(n_units, n_walkers):
    """Unit u goes to walker u % n_walkers: -> the trip count of every walker."""
    return [len(range(w, n_units, n_walkers)) for w in range(n_walkers)]


def edge_trips(n_items, hd, cap):
    """The trips of every wave of the group-per-row backward at the largest G this H*D allows (a smaller G: more trips)."""
    g = group_items_max(hd)
    return strided_trips((n_items + g - 1) // g, WAVES * edge_blocks(n_items, cap))


def row_shape(hd, norm):
    """(lanes per row, rows per block) of res_backward_shape / norm_backward_shape (gat_dense_kernels.hip:346, :370) and hidden_shape
    (gat_head_hidden.hip:134, the res_backward rule)."""
    groups = hd // 4 if hd % 4 == 0 else hd
    if norm:
        lpr = 1
        while lpr < groups and lpr < 64:
            lpr <<= 1
    else:
        lpr = min(groups, 256)
    return lpr, 256 // lpr


def row_trips(n_rows, rows_per_trip, cap):
    """A row kernel whose block takes rows_per_trip rows a trip on min(tiles, cap) blocks -> (trips per block, rows of the last tile)."""
    tiles = max(1, -(-n_rows // rows_per_trip))
    return strided_trips(tiles, min(tiles, cap)), n_rows - (tiles - 1) * rows_per_trip


# -- the graphs
NARROW_ROWS = {23: 32, 57: 15, 130: 33, 211: 16, 302: 31, 377: 17}
NARROW_HUB = (7, 300)
NARROW_EMPTY = (3, 400)
NARROW_N = 401


def narrow_graph():
    """401 nodes, F = 24, C = 5, about 900 edges: a hub row of 300 in-edges, rows of 15, 16, 17, 31, 32 and 33 in-edges at scattered row
    numbers, two empty rows (one the last), every other row one or two in-edges.  For the models of H*D = 16 and 8, whose waves hold 16
    and 32 items: more than 385 items at 16-edge segments, and few enough values that seeds clear of the kinks exist.  401 rows: no
    row kernel's tile (16, 17, 64, 128 rows) divides them."""
    rng = np.random.default_rng(23)
    n, F, C = NARROW_N, 24, 5
    deg = rng.choice([1, 2], n, p=[0.8, 0.2])
    for r, d in NARROW_ROWS.items():
        deg[r] = d
    deg[NARROW_HUB[0]] = NARROW_HUB[1]
    deg[list(NARROW_EMPTY)] = 0
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    src = rng.integers(0, n, int(rp[-1]))
    ci = np.concatenate([np.sort(src[rp[r]:rp[r + 1]]) for r in range(n)]).astype(np.int32)
    x = rng.standard_normal((n, F)).astype(np.float32)
    lab = rng.integers(0, C, n).astype(np.int32)
    return dict(row_ptr=rp, col_idx=ci, x=x, labels=lab, n=n, f=F, c=C)


_GRAPHS = {}


def graph(name):
    """(name, graph dict): the graph argument of pick_profiles.run_case."""
    if name not in _GRAPHS:
        _GRAPHS[name] = {"parity": FC.parity_graph, "narrow": narrow_graph}[name]()
    return name, _GRAPHS[name]


def n_items(g):
    split, whole = PP.worklist(g["row_ptr"], SEG)
    return len(split) + len(whole)


# -- the edge forms: pick_profiles' case tuples (model name, heads, outdims, storage, form, edge_dim) and the graph of each
HD16 = ("hd16_d8", [2, 2], [8, 8], "fp32")
NARROW_MODELS = ("hd16_d8", "hd8_d4", "generic")         # H*D <= 16 (generic: 15 and 16): the row count goes up as H*D goes down


def graph_of(case):
    return "narrow" if case[0] in NARROW_MODELS else "parity"


def fast_hd(case):
    """The H*D of the layers on the persistent (listed-shape) backward kernels; the generic kernel takes a row per block."""
    return [h * d for h, d in zip(case[1], case[2]) if (h * d, d) in FC.SHAPES]


EDGE_CASES = list(PP.CASES)
EDGE_CASES += [(*HD16, form, 0) for form in PP.PLAIN_FORMS if form != "taps_res_norm_reg"]
EDGE_CASES += [(*HD16, form, PP.FE) for form in ("plain", "res_norm_reg")]
# the wave-per-row kernels take the forms without a mask and without the edge term (pick_bwd: the DROP / PE instantiations are the
# group-per-row kernel's whatever the A/B switches say): fp32 records and message rows, and the bf16 message rows of H*D = 32 — the one
# layer GAT_GROUP_MSG decides (bf16 records have no wave-per-row form)
WAVE_ROW_CASES = [c for c in EDGE_CASES if c[4] in ("plain", "res_norm") and c[5] == 0]
# the fused last layer takes (8, 8), C <= 64, fp32 and no feature form: the plain model against fp64, and the fused children of
# tests/test_output_head.py (training masks on and off, the head's outputs against head_ref on the tapped rows)
FUSED_EDGE_CASES = [c for c in EDGE_CASES if c[0] == "hd64_d8" and c[3] == "fp32" and c[4] == "plain" and c[5] == 0]
FUSED_HEAD_CASES = [c for c in HC.CHILDREN["GAT_FUSE_LAST=1"][1] if c.C > 1]

# -- the heads
N_RAND = 247                                             # pair_ref.pair_list: 262 hub pairs + 247 random + 4 = 513 pairs
N_PAIRS = 513                                            # four 128-row tiles and a ragged fifth
HEAD_FAMILIES = ("records_d8", "generic")
HEAD_MLP_CASES = [c for c in HM.cases() if c[0] in HEAD_FAMILIES]
PAIR_CASES = [c for c in PR.cases(FC) if c[0] in HEAD_FAMILIES]
# BCE / MSE: the whole step at D_last = 4, 8, 16 and an any-shape D_last (generic: 8 behind a 15-wide layer runs the any-shape kernels of
# the loss head at D_last = 8; (4, 5) below is the any-shape D_last of the head alone), the feature stack and the mask on records_d8
LOSS_STEP_CASES = [c for c in LR.step_cases(FC) if c[0] in ("records_d4", "records_d8", "msg_rows_d16", "generic")]
LOSS_HEAD_ROWS = 300                                     # two tiles and a ragged third, masked (tests/test_loss_modes.py HEAD_ROWS)
LOSS_HEAD_CASES = [(C, last, mode, how) for C in (3, 65) for last in ((8, 4), (8, 8), (4, 16), (4, 5)) for mode in LR.MODES
                   for how in ("step", "fwdbwd")]
# the softmax head: the D_last sweep at C = 7 and the mask cases (N140001 is left out: one block would walk 1094 tiles)
SOFTMAX_HEAD_CASES = [c for c in HC.CASES if (c.name.startswith("C7-h") and c.layers == 1) or c.name.startswith("mask-")]
SEAM_CASES = [(which, w) for which in ("forward", "backward") for w in (1, 3, 4, 5, 16, 64, 65, 80, 256)]


def _edge(case):
    return lambda pkg, orc: PP.run_case(pkg, orc, case, graph(graph_of(case)))


def _head_mlp(case):
    def run(pkg, orc):
        import test_head_mlp as T                        # its compare_all: the comparison of the parent test, not a copy
        ci = HM.case_inputs(case, N_RAND)
        assert ci["rows"] == (N_PAIRS if case[2].startswith("pair") else ci["rows"])
        ref = HM.model_of(ci)
        with HM.make_ctx(pkg, ci) as ctx:
            loss, correct = ctx.step()
            T.compare_all(pkg, ctx, ci, ref, loss, 1e-2 if ci["bf16"] else 1e-4)
            if ci["loss"] == HM.SOFTMAX and not ci["bf16"]:
                keep = np.ones(ci["rows"], bool) if ci["mask"] is None else ci["mask"]
                assert correct == int(((np.argmax(ref["y"], axis=1) == ci["sup"]) & keep).sum())
    return run


def _pair(case):
    def run(pkg, orc):
        import test_pair_head as T
        ci = PR.case_inputs(case, N_RAND)
        assert len(ci["u"]) == N_PAIRS
        ref = PR.model_of(ci)
        with PR.make_ctx(pkg, ci) as ctx:
            loss, correct = ctx.step()
            T.compare_all(pkg, ctx, ci, ref, loss, 1e-2 if ci["bf16"] else 1e-4)
            if ci["loss"] == PR.SOFTMAX and not ci["bf16"]:
                keep = np.ones(N_PAIRS, bool) if ci["mask"] is None else ci["mask"]
                assert correct == int(((np.argmax(ref["y"], axis=1) == ci["sup"]) & keep).sum())
    return run


def _loss_step(case):
    def run(pkg, orc):
        import test_loss_modes as T
        ci = LR.step_inputs(case)
        ref = LR.model_of(ci)
        with LR.make_ctx(pkg, ci) as ctx:
            loss, correct = ctx.step()
            T.compare_step(pkg, ctx, ci, ref, loss, 1e-2 if ci["bf16"] else parity.TOL)
            T.check_count(pkg, ctx, ci, correct, ci["mask"])
    return run


def _loss_head(case):
    def run(pkg, orc):
        import test_loss_modes as T
        C, last, mode, how = case
        out, ref = T.run_head_case(pkg, C, last, LOSS_HEAD_ROWS, mode, how)
        T.check_head(out, ref, mode)
    return run


def _seam(case):
    def run(pkg, orc):
        import torch
        import test_head_mlp as T                        # the seam laws of the parent test: forward bitwise, gA bitwise, gradb1 in its bound
        which, width = case
        fn = T.test_seam_forward_is_bitwise if which == "forward" else T.test_seam_backward_bitwise_and_within_the_summation_bound
        fn(pkg, (torch, torch.device("cuda:0")), width)
    return run


def table(profile):
    """[(case id, run(pkg, orc))] of a profile, in a fixed order."""
    if profile == "cap1_fused":
        out = [("edge " + PP.case_id(c), _edge(c)) for c in FUSED_EDGE_CASES]
        return out + [("head " + c.name, (lambda c: lambda pkg, orc: HC.run_case(pkg, c))(c)) for c in FUSED_HEAD_CASES]
    if profile == "cap1_wave_rows":
        return [("edge " + PP.case_id(c), _edge(c)) for c in WAVE_ROW_CASES]
    out = [("edge " + PP.case_id(c), _edge(c)) for c in EDGE_CASES]
    out += [("head_mlp " + HM.case_id(c), _head_mlp(c)) for c in HEAD_MLP_CASES]
    out += [("pair " + PR.case_id(c), _pair(c)) for c in PAIR_CASES]
    out += [("loss " + LR.case_id(c), _loss_step(c)) for c in LOSS_STEP_CASES]
    out += [("loss_head C%d-h%dd%d-%s-%s" % (c[0], *c[1], c[2], c[3]), _loss_head(c)) for c in LOSS_HEAD_CASES]
    out += [("softmax_head " + c.name, (lambda c: lambda pkg, orc: HC.run_case(pkg, c))(c)) for c in SOFTMAX_HEAD_CASES]
    out += [("seam %s w%d" % c, _seam(c)) for c in SEAM_CASES]
    return out


def run_profile(pkg, orc, profile):
    """Every case of the profile's table in this process (whose environment is the profile's).  A failing case does not stop the
    others: it is printed with its profile and case, and the achieved errors of all cases are written out.  -> (cases, failures)"""
    failures = []
    cases = table(profile)
    for name, run in cases:
        parity.set_test(f"grid trips {profile}: {name}")
        try:
            run(pkg, orc)
        except Exception as e:      # noqa: BLE001 - a refused launch or a bad shape is a failure of that case like a missed bar
            failures.append(f"{profile}: {name}: {type(e).__name__}: {e}")
            print("FAILED", failures[-1], flush=True)
    parity.flush()
    return len(cases), failures
