"""What tests/test_grid_trips.py relies on, proved on the host: under the profiles of tests/trip_cases.py every persistent kernel of every
case walks several trips (three full ones and a ragged fourth for the edge kernels; at least three with a ragged last one for the row
kernels, two for the 128-row head tiles of the node kinds), GAT_RESIDENT_CAP=3 gives the blocks of every kernel family unequal trip
counts somewhere, the graphs have the rows they claim, and every case has a parameter seed clear of the kinks.  The trip counts come
from the launchers' rules as tests/trip_cases.py restates them (the source lines are named there)."""
import numpy as np
import pytest

import feature_cases as FC
import head_cases as HC
import head_mlp_ref as HM
import loss_ref as LR
import pair_ref as PR
import pick_profiles as PP
import trip_cases as TC


def test_profiles():
    assert TC.PROFILES == {
        "cap1": {"GAT_RESIDENT_CAP": "1"},
        "cap3": {"GAT_RESIDENT_CAP": "3"},
        "cap1_fused": {"GAT_RESIDENT_CAP": "1", "GAT_FUSE_LAST": "1"},
        "cap1_wave_rows": {"GAT_RESIDENT_CAP": "1", "GAT_ROWGROUP": "0", "GAT_GROUP_MSG": "0"},
    }
    assert set(TC.TIMEOUT) == set(TC.PROFILES) and max(TC.TIMEOUT.values()) < 900


# -- the graphs
def test_narrow_graph_has_what_it_claims():
    g = TC.narrow_graph()
    rp = g["row_ptr"]
    deg = np.diff(rp)
    assert (g["n"], g["f"], g["c"]) == (401, 24, 5) and g["x"].shape == (401, 24) and len(g["labels"]) == 401
    assert 850 <= rp[-1] <= 950 and len(g["col_idx"]) == rp[-1]
    assert g["col_idx"].min() >= 0 and g["col_idx"].max() < g["n"]
    for r in range(g["n"]):                                                  # sources ascending inside a row
        assert np.all(np.diff(g["col_idx"][rp[r]:rp[r + 1]]) >= 0)
    assert deg[TC.NARROW_HUB[0]] == 300
    assert sorted(TC.NARROW_ROWS.values()) == [15, 16, 17, 31, 32, 33]
    for r, d in TC.NARROW_ROWS.items():
        assert deg[r] == d
    rows = sorted(TC.NARROW_ROWS)
    assert min(np.diff(rows)) > 30                                           # scattered, and in no order of length
    assert [TC.NARROW_ROWS[r] for r in rows] != sorted(TC.NARROW_ROWS.values())
    assert np.flatnonzero(deg == 0).tolist() == list(TC.NARROW_EMPTY) and TC.NARROW_EMPTY[-1] == g["n"] - 1
    assert TC.n_items(g) >= 385
    split, whole = PP.worklist(rp, TC.SEG)
    assert len(split) == 19 + 2 + 2 + 2 + 3                                  # the hub, 17, 31, 32, 33
    for tile in (16, 17, 64, 128):                                           # the row tiles of the H*D = 8, 15, 16 row kernels
        assert g["n"] % tile != 0


def test_parity_graph_is_the_one_the_counts_assume():
    g = FC.parity_graph()
    assert g["n"] == 150 and TC.n_items(g) >= TC.items_needed(32)            # 97 at H*D = 32, 49 at 64


# -- the edge kernels
@pytest.mark.parametrize("case", TC.EDGE_CASES, ids=[PP.case_id(c) for c in TC.EDGE_CASES])
def test_edge_case_walks_and_has_a_seed(orc, case):
    name, g = TC.graph(TC.graph_of(case))
    n = TC.n_items(g)
    hds = TC.fast_hd(case)
    assert hds, "no layer on the persistent kernels"
    for hd in hds:
        G = TC.group_items_max(hd)
        assert hd % TC.MAX_N == 0 and G * (hd // TC.MAX_N) == 64 and G <= 256 // hd          # LPE = H*D / N lanes an item, G items a wave
        assert n >= TC.items_needed(hd) == 3072 // hd + 1, (name, n, hd)
        trips = TC.edge_trips(n, hd, 1)
        assert len(trips) == TC.WAVES and max(trips) >= 4 and (min(trips) < max(trips) or n % G), (trips, n, G)
    if case in TC.WAVE_ROW_CASES:                                            # the wave-per-row kernels: an item per wave and trip
        assert min(TC.strided_trips(n, TC.WAVES * TC.edge_blocks(n, 1))) >= 4
    out = PP.reference(orc, case, (name, g))                                 # the seed search of the parent tests: fails without a seed
    assert 0 <= out[-1]["seed"] < 40


def test_edge_tables():
    ids = [PP.case_id(c) for c in TC.EDGE_CASES]
    assert len(set(ids)) == len(ids)
    assert all(c in TC.EDGE_CASES for c in PP.CASES)                             # every form of the full-size table ...
    models = {c[0] for c in TC.EDGE_CASES}
    assert {m[0] for m in PP.MODELS} | {"generic", "hd16_d8"} == models      # ... on every model, generic and an H*D = 16 one
    hd_narrow = {hd for c in TC.EDGE_CASES if TC.graph_of(c) == "narrow" for hd in TC.fast_hd(c)}
    assert hd_narrow == {16, 8}
    assert {c[3] for c in TC.EDGE_CASES} == {"fp32", "bf16"}
    assert sum(c[4] == "taps_res_norm_reg" for c in TC.EDGE_CASES) == 2 and all(c[0] == "hd64_d8" for c in TC.EDGE_CASES if c[4] == "taps_res_norm_reg")
    assert sum(c[5] == PP.FE for c in TC.EDGE_CASES) == 2 * (len(PP.MODELS) + 1)
    assert all(not PP.PLAIN_FORMS[c[4]][1] and c[5] == 0 for c in TC.WAVE_ROW_CASES)                 # no DROP / PE instantiation
    assert {c[2][0] for c in TC.WAVE_ROW_CASES if c[3] == "fp32"} >= {4, 8, 16}                      # records and message rows
    assert any(c[0] == "hd32_d8" and c[3] == "bf16" for c in TC.WAVE_ROW_CASES)                      # GAT_GROUP_MSG is read there
    assert [PP.case_id(c) for c in TC.FUSED_EDGE_CASES] == ["hd64_d8-fp32-plain"]


def test_fused_cases_walk():
    """The fused last layer: four items per wave, sixteen per block and trip (edge_last_fused_blocks), over the unsplit rows."""
    assert {c.masked for c in TC.FUSED_HEAD_CASES} == {False, True}
    for c in TC.FUSED_HEAD_CASES:
        assert c.last == (8, 8) and c.C <= 64 and c.dtype == "f32" and c.expect_fused
        split, whole = PP.worklist(HC.make_inputs(c)["rp"], TC.SEG)
        assert len(split) >= 2 and len(whole) >= 3 * 16 + 1 and len(whole) % 16 != 0, (c.name, len(whole))
    g = FC.parity_graph()
    split, whole = PP.worklist(g["row_ptr"], TC.SEG)
    assert len(whole) >= 3 * 16 + 1 and len(whole) % 16 != 0


# -- the row kernels under the edge cases: res_backward, norm_backward
@pytest.mark.parametrize("case", [c for c in TC.EDGE_CASES if PP.PLAIN_FORMS[c[4]][0]], ids=lambda c: PP.case_id(c))
def test_row_kernels_walk(case):
    n = TC.graph(TC.graph_of(case))[1]["n"]
    for h, d in zip(case[1], case[2]):
        for norm in (False, True):
            lpr, rpb = TC.row_shape(h * d, norm)
            assert lpr * rpb <= 256
            trips, last = TC.row_trips(n, rpb, 1)
            assert trips[0] >= 3 and 0 < last < rpb, (h * d, norm, rpb, trips, last)


# -- the heads
def tiles(rows, cap=1):
    return TC.row_trips(rows, TC.HEAD_TILE, cap)


def test_pair_lists():
    u, v = PR.pair_list(150, n_rand=TC.N_RAND)
    assert len(u) == len(v) == TC.N_PAIRS >= 513
    trips, last = tiles(TC.N_PAIRS)
    assert trips == [5] and last == 1                                        # four 128-row tiles and a ragged fifth
    assert all(c[0] in TC.HEAD_FAMILIES for c in TC.HEAD_MLP_CASES + TC.PAIR_CASES)
    assert {c[2] for c in TC.HEAD_MLP_CASES} == set(HM.KINDS) and {c[3] for c in TC.HEAD_MLP_CASES} == {HM.SOFTMAX, HM.BCE, HM.MSE}


@pytest.mark.parametrize("case", TC.HEAD_MLP_CASES, ids=[HM.case_id(c) for c in TC.HEAD_MLP_CASES])
def test_head_mlp_case_walks_and_has_a_seed(orc, case):
    ci = HM.case_inputs(case, TC.N_RAND)                                     # fails without a clear seed
    kind, dh = case[2], case[4]
    if kind.startswith("pair"):
        assert ci["rows"] == TC.N_PAIRS
        trips, last = tiles(ci["rows"])
        assert trips[0] >= 3 and 0 < last < TC.HEAD_TILE
        lpr, rpb = TC.row_shape(dh, False)                                   # the hidden layer: rpb * kU rows a trip
        trips, last = TC.row_trips(ci["rows"], rpb * TC.K_U, 1)
        assert trips[0] >= 3 and 0 < last < rpb * TC.K_U, (dh, rpb, trips, last)
        if dh == 16:
            assert rpb * TC.K_U == 256 and trips == [3]
    elif kind == "node":
        trips, last = tiles(ci["rows"])
        assert trips[0] >= 2 and 0 < last < TC.HEAD_TILE
    else:                                                                    # readout: the head's rows are the five graphs, one tile;
        assert ci["rows"] == len(ci["graph_ptr"]) - 1                        # the trips are those of the node model under it
        assert tiles(ci["g"]["n"])[0][0] >= 2


@pytest.mark.parametrize("case", TC.PAIR_CASES, ids=[PR.case_id(c) for c in TC.PAIR_CASES])
def test_pair_case_has_a_seed(orc, case):
    ci = PR.case_inputs(case, TC.N_RAND)
    assert len(ci["u"]) == TC.N_PAIRS and 0 <= ci["seed"] < 40


def test_loss_cases_walk_and_have_seeds(orc):
    assert {c[0] for c in TC.LOSS_STEP_CASES} == {"records_d4", "records_d8", "msg_rows_d16", "generic"}
    assert {c[2] for c in TC.LOSS_STEP_CASES} == set(LR.MODES) and {c[1] for c in TC.LOSS_STEP_CASES} == {"plain", "res_norm_reg", "mask"}
    for c in TC.LOSS_STEP_CASES:
        ci = LR.step_inputs(c)                                               # fails without a clear seed
        trips, last = tiles(ci["g"]["n"])
        assert trips[0] >= 2 and 0 < last < TC.HEAD_TILE
    assert {c[1][1] for c in TC.LOSS_HEAD_CASES} == {4, 8, 16, 5} and {c[2] for c in TC.LOSS_HEAD_CASES} == set(LR.MODES)
    trips, last = tiles(TC.LOSS_HEAD_ROWS)
    assert trips == [3] and 0 < last < TC.HEAD_TILE


def test_softmax_head_cases_walk():
    names = [c.name for c in TC.SOFTMAX_HEAD_CASES]
    assert "N140001" not in names
    assert sum(n.startswith("mask-") for n in names) == sum(c.name.startswith("mask-") for c in HC.CASES) > 0
    assert [c.last for c in TC.SOFTMAX_HEAD_CASES if not c.name.startswith("mask-")] == HC.D_SHAPES
    for c in TC.SOFTMAX_HEAD_CASES:
        trips, last = tiles(c.n)
        assert trips[0] >= 2 and 0 < last < TC.HEAD_TILE, c.name


def test_seams_walk():
    """gat_op_head_hidden_*: 1000 rows under cap 1.  Widths 1 and 4 put one lane on a row — 1024 rows a trip, a single ragged trip —
    every other width walks at least three."""
    widths = sorted({w for _, w in TC.SEAM_CASES})
    assert widths == [1, 3, 4, 5, 16, 64, 65, 80, 256] and len(TC.SEAM_CASES) == 2 * len(widths)
    for w in widths:
        lpr, rpb = TC.row_shape(w, False)
        trips, last = TC.row_trips(1000, rpb * TC.K_U, 1)
        if w in (1, 4):
            assert rpb * TC.K_U == 1024 and trips == [1]
        else:
            assert trips[0] >= 3 and 0 < last < rpb * TC.K_U, (w, trips, last)


# -- cap 3: unequal trip counts in every kernel family
def test_cap3_gives_unequal_trip_counts():
    unequal = lambda t: len(t) == 3 * (len(t) // 3) and min(t) < max(t)
    n = TC.n_items(FC.parity_graph())
    groups = TC.edge_trips(n, 64, 3)
    assert len(groups) == 12 and unequal(groups)                             # group-per-row: 12 waves
    m = TC.n_items(TC.narrow_graph())                                        # wave-per-row: parity_graph's 168 items deal evenly on 12 waves
    assert unequal(TC.strided_trips(m, TC.WAVES * TC.edge_blocks(m, 3)))
    for norm in (False, True):                                               # res_backward, norm_backward at H*D = 64
        trips, _ = TC.row_trips(150, TC.row_shape(64, norm)[1], 3)
        assert len(trips) == 3 and unequal(trips)
    trips, _ = tiles(TC.N_PAIRS, 3)                                          # the heads: five tiles on three blocks
    assert trips == [2, 2, 1]
    trips, _ = TC.row_trips(TC.N_PAIRS, TC.row_shape(24, False)[1] * TC.K_U, 3)      # the hidden layer at width 24: four trips on three blocks
    assert len(trips) == 3 and unequal(trips)
    trips, _ = TC.row_trips(1000, TC.row_shape(16, False)[1] * TC.K_U, 3)    # its seams at width 16
    assert unequal(trips)


def test_tables_are_what_the_gpu_test_counts():
    for profile in TC.PROFILES:
        ids = [name for name, _ in TC.table(profile)]
        assert len(ids) == len(set(ids)) > 0, profile
    assert len(TC.table("cap1")) == len(TC.table("cap3")) == (len(TC.EDGE_CASES) + len(TC.HEAD_MLP_CASES) + len(TC.PAIR_CASES) + len(TC.LOSS_STEP_CASES)
                                                              + len(TC.LOSS_HEAD_CASES) + len(TC.SOFTMAX_HEAD_CASES) + len(TC.SEAM_CASES))
    assert len(TC.table("cap1_fused")) == len(TC.FUSED_EDGE_CASES) + len(TC.FUSED_HEAD_CASES)
    assert len(TC.table("cap1_wave_rows")) == len(TC.WAVE_ROW_CASES)
