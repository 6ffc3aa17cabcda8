"""tests/test_full_size_picks.py without a GPU: the profile table follows from the library's rules and the BASELINE shapes; the graph has
the rows the profiles treat differently — and, at the suite's default segment length, none of them unsplit: the gap the GPU module
closes; the masks of REG reach the positions and the all-dropped steps of long rows; every case has a parameter seed clear of the
LeakyReLU kinks (a condition on the inputs, proven by the reference alone)."""
import json
import os

import numpy as np
import pytest

import feature_cases as FC
import pick_profiles as PP
from feature_cases import REG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGS = (32, 64, 256)
U = 4                                            # edges per step of the group-per-row kernels


# -- 1. the profiles
def test_rules_at_their_thresholds():
    assert [PP.seg_edges(e) for e in (0, (512 << 10) - 1, 512 << 10, (4 << 20) - 1, 4 << 20, (16 << 20) - 1, 16 << 20)] == [16, 16, 32, 32, 64, 64, 256]
    assert not PP.short_lists_take_runs((512 << 10) - 1, 1 << 20) and PP.short_lists_take_runs(512 << 10, 1 << 20)
    assert PP.short_lists_take_runs(8 * 100_000 - 1, 100_000) and not PP.short_lists_take_runs(8 * 100_000, 100_000)
    mb = 1 << 20
    assert not PP.node_records(128 * mb // 256, 64, False, False) and PP.node_records(128 * mb // 256 + 1, 64, False, False)
    assert not PP.node_records(64 * mb // 256, 64, True, False) and PP.node_records(64 * mb // 256 + 1, 64, True, False)
    assert not PP.node_records(1 << 25, 64, False, True)                 # bf16 storage keeps no node records


def test_profiles_follow_from_the_baseline_shapes():
    configs = " | ".join(json.load(open(os.path.join(ROOT, "BASELINE.json")))["configs"])
    assert sorted(PP.PROFILES) == sorted(PP.PROFILE_SHAPES)
    for name, (n_rows, n_table, n_edges, hd, bf16, text) in PP.PROFILE_SHAPES.items():
        assert text in configs, name
        assert PP.profile_env(n_rows, n_table, n_edges, hd, bf16) == PP.PROFILES[name], name
    # the P = 8 shard: an eighth of the Products rows and edges (about 306 k rows, 7.7 M edges, 78 MB of g rows), the whole table
    n_rows, n_table, n_edges = PP.PROFILE_SHAPES["products_p8"][:3]
    assert (n_rows, n_table) == (306_250, 2_450_000) and 7.7e6 < n_edges < 7.8e6 and (64 << 20) < 78e6 < n_rows * 256 < 79e6 < (128 << 20)
    # spelled out: segment length, pull family, node records
    picks = {name: (PP.seg_edges(s[2]), PP.short_lists_take_runs(s[2], s[1]), PP.node_records(s[0], s[3], PP.short_lists_take_runs(s[2], s[1]), s[4]))
             for name, s in PP.PROFILE_SHAPES.items()}
    assert picks == {"products": (256, False, True), "arxiv": (32, True, False), "products_p8": (64, True, True), "config5": (256, False, False)}
    # the small graph's own defaults: segments of 16, list pull, no node records — no profile is the suite's default
    g = PP.long_rows_graph()
    e = len(g["col_idx"])
    assert PP.profile_env(g["n"], g["n"], e, 64, False) == {"GAT_SEG_EDGES": "16", "GAT_PULL_LAST": "0"}
    assert len({tuple(sorted(env.items())) for env in PP.PROFILES.values()}) == 4
    for env in PP.PROFILES.values():             # nothing else is set: the heavy-chunk threshold and the sort window stay the production ones
        assert set(env) <= {"GAT_SEG_EDGES", "GAT_PULL_RUNS", "GAT_PULL_LAST"}


# -- 2. the graph
def test_the_graph_has_the_rows():
    g = PP.long_rows_graph()
    rp, ci = g["row_ptr"], g["col_idx"]
    deg = np.diff(rp)
    assert g["n"] == 96 and g["f"] == 24 and g["c"] == 5 and len(ci) == rp[-1] and len(ci) < (512 << 10)
    longs = sorted(d for d in deg if d > 5)
    assert longs == [15, 16, 17, 31, 32, 33, 63, 64, 65, 256, 257] == sorted(PP.LONG_ROWS.values())
    assert all(deg[r] == d for r, d in PP.LONG_ROWS.items())
    assert [r for r in range(96) if deg[r] == 0] == [3, 95]
    assert all(1 <= d <= 5 for r, d in enumerate(deg) if r not in PP.LONG_ROWS and r not in PP.EMPTY_ROWS)
    by_row = [PP.LONG_ROWS[r] for r in sorted(PP.LONG_ROWS)]
    assert by_row != sorted(by_row) and by_row != sorted(by_row, reverse=True)           # in no order of length
    assert ci.min() >= 0 and ci.max() < 96 and all((np.diff(ci[rp[r]:rp[r + 1]]) >= 0).all() for r in range(96))
    hub = int((ci == PP.HUB).sum())
    assert hub > 256 and 0.25 < hub / len(ci) < 0.35                                    # the chunk kernels at the production threshold
    assert np.bincount(ci, minlength=96).argsort()[-2:].tolist()[1] == PP.HUB


@pytest.mark.parametrize("seg", SEGS)
def test_work_list_of_a_full_size_segment_length(seg):
    rp = PP.long_rows_graph()["row_ptr"]
    split, whole = PP.worklist(rp, seg)
    lens = [e - b for _, b, e in whole]
    assert max(lens) == seg and sum(n > 16 for n in lens) >= 2                           # unsplit items above 16 edges, one exactly a segment
    last = {}
    for r, b, e in split:
        assert 0 < e - b <= seg
        last[r] = e - b
    assert 1 in last.values()                                                           # a split row whose last segment holds one edge
    assert sum(e - b for _, b, e in split + whole) == rp[-1] and len(whole) + len(last) == 96
    assert lens == sorted(lens, reverse=True)
    # unequal neighbours: a wave of the group-per-row kernels carries 4 (H*D = 64, D = 8) to 16 (H*D = 8, D = 4) consecutive items and
    # walks to the longest; somewhere an item above 16 edges shares its wave with one a step or more shorter, which idles on clamped indices
    items = [e - b for _, b, e in split + whole]
    for G in (4, 8, 16):
        waves = [items[i:i + G] for i in range(0, len(items), G)]
        assert any(max(w) > 16 and (max(w) + U - 1) // U > (min(w) + U - 1) // U for w in waves), G


def test_the_default_work_list_never_walks_more_than_16_edges():
    """The statement of the gap: at the segment length this graph (and every graph of the suite) takes by default, no item of the
    group-per-row kernels exceeds 16 edges — four steps — and no row above 16 edges is closed in the kernels' own epilogue."""
    g = PP.long_rows_graph()
    assert PP.seg_edges(len(g["col_idx"])) == 16
    split, whole = PP.worklist(g["row_ptr"], 16)
    assert max(e - b for _, b, e in split + whole) == 16
    assert {r for r, _, _ in split} == {r for r, d in PP.LONG_ROWS.items() if d > 16}
    for graph in (FC.parity_graph(), FC.make_graph(1), FC.host_graph(1), FC.wide_graph(), FC.shard_problem()):
        assert PP.seg_edges(len(graph["col_idx"])) == 16


# -- 3. the masks
@pytest.mark.parametrize("seg", SEGS)
def test_masks_cover_the_long_rows(orc, seg):
    """Under REG, in rows that are ONE item at this segment length: a step of four edges 4k .. 4k+3, all dropped by DropEdge, at a
    position of 16 or above (cm = -inf inside the online softmax of a long walk), with kept edges before and after it in the row; and
    the DropEdge and attention masks at positions 16 and above are not those of the positions 16 lower (an item-relative or wrapped
    position would draw another mask)."""
    g = PP.long_rows_graph()
    rp = g["row_ptr"]
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    keeps, attn, _ = FC.masks(cfg, g, cfg.heads, REG)
    _, whole = PP.worklist(rp, seg)
    rows = [(b, e) for _, b, e in whole if e - b > 16]
    assert rows
    for l in range(cfg.L):
        dead = 0
        for b, e in rows:
            k = keeps[l][b:e]
            for p in range(16, e - b - U + 1, U):
                dead += (not k[p:p + U].any()) and k[:p].any() and k[p + U:].any()
        assert dead > 0, (seg, l)
        for name, m in (("edge", keeps[l][None, :]), ("attn", attn[l] != 0)):
            assert any((m[:, b + 16:e] != m[:, b:e - 16]).any() for b, e in rows), (name, l)
            assert any(m[:, b:b + 16].any() and not m[:, b + 16:e].all() and m[:, b + 16:e].any() for b, e in rows), (name, l)


# -- 4. the seeds
MODELS = sorted({(c[0], tuple(c[1]), tuple(c[2]), c[3], PP.PLAIN_FORMS[c[4]][0], PP.PLAIN_FORMS[c[4]][1], c[5]) for c in PP.CASES})


def test_case_table():
    assert len(PP.CASES) == 48 and len({PP.case_id(c) for c in PP.CASES}) == 48 and len(MODELS) == 46
    assert sum(c[4] == "taps_res_norm_reg" for c in PP.CASES) == 2 and sum(c[5] == PP.FE for c in PP.CASES) == 14
    assert {c[3] for c in PP.CASES if c[0] == "generic"} == {"fp32"}


@pytest.mark.parametrize("model", MODELS, ids=[f"{m[0]}-{m[3]}-norm{int(m[4])}-reg{int(m[5])}-fe{m[6]}" for m in MODELS])
def test_some_seed_is_clear_of_the_kink(orc, model):
    """FC.pick_params raises when none of its seeds keeps the model off the kinks."""
    name, heads, outdims, dt, norm, reg, fe = model
    form = next(f for f, v in PP.PLAIN_FORMS.items() if v[:2] == (norm, reg))
    P, inp, ref = PP.reference(orc, (name, list(heads), list(outdims), dt, form, fe))
    assert 0 <= ref["seed"] < 40 and np.isfinite(ref["loss"].item())
