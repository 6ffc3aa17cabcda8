"""tests/test_edge_shapes.py without a GPU: which kernel instantiation each of its 112 cases reaches (COVERAGE, restated from pick_fwd /
pick_bwd of csrc/gat_edge_kernels.hip and the record-path rule of csrc/gat_abi.hip (ensure_buffers) — documentation that cannot silently shrink, it
inspects no binary), the `alpha` key of tests/step_ref.py, and — a condition, not a skip — a parameter seed clear of the
LeakyReLU kinks among the first 40 for every case of the matrix."""
import re

import numpy as np
import pytest

import feature_cases as T
from feature_cases import REG, masks, parity_graph


def stash_n(hd, d):
    """Channels per lane of the two-lanes-per-head (group-per-row) kernels of a shape, 0: the shape has none (stash_n of the .hip)."""
    return 4 if (d == 8 and hd >= 32) else (2 if d == 4 else 0)


def picks(hd, d, bf16, form):
    """-> (forward, fix-up, backward) kernel of a case at the default settings.
    Forward: every form runs a DROP instantiation (a residual / norm context with nothing dropped runs it at T = 0); keep_taps: the
    ALPHA form of the one-channel-per-lane kernel, else the group-per-row kernel where the shape has one, else the packed one.
    Fix-up of the split rows: the RES form in a residual / norm context.
    Backward: the DROP instantiation while a regulariser draws a mask, else the default pick.  A layer keeps per-edge records
    (stash) where the shape has a record path, not with keep_taps, and with bf16 storage only at H*D = 64."""
    norm, reg, taps = T.FORMS[form]
    n3, n2 = stash_n(hd, d), (4 if hd >= 32 and d % 4 == 0 else 2)
    bf = "true" if bf16 else "false"
    alpha = "true" if taps else "false"
    if taps:
        fwd = f"edge_fwd_kernel<{hd}, {d}, true, {bf}, true>"
    elif n3:
        fwd = f"edge_fwd3_kernel<{hd}, {d}, {n3}, {bf}, true>"
    else:
        fwd = f"edge_fwd2_kernel<{hd}, {d}, {n2}, {bf}, true>"
    fix = f"edge_fwd_fix_kernel<{hd}, {d}, {alpha}, true>" if norm else f"edge_fwd_fix_kernel<{hd}, {d}, {alpha}>"
    stash = n3 != 0 and not taps and not (bf16 and hd < 64)
    if reg:
        if taps:
            bwd = f"edge_bwd_kernel<{hd}, {d}, true, true, 0, {bf}, true>"
        elif n3:
            bwd = f"edge_bwd3_kernel<{hd}, {d}, {n3}, 0, {bf}, {'false' if stash else 'true'}, true>"
        else:
            bwd = f"edge_bwd2_kernel<{hd}, {d}, {n2}, 0, {bf}, false, true>"
    else:
        assert not taps
        if n3:
            bwd = f"edge_bwd3_kernel<{hd}, {d}, {n3}, 0, {bf}>" if stash else f"edge_bwd3_kernel<{hd}, {d}, {n3}, 0, {bf}, true>"
        else:
            bwd = f"edge_bwd2_kernel<{hd}, {d}, {n2}, 0, {bf}>"
    return fwd, fix, bwd


COVERAGE = {(hd, d, bf16, form): picks(hd, d, bf16, form)
            for hd, d in [(64, 8), (64, 4), (64, 16), (64, 32), (64, 64), (32, 8), (32, 4), (32, 16), (32, 32), (16, 4), (16, 8), (16, 16),
                          (8, 4), (8, 8)]
            for bf16 in (False, True)
            for form in ("reg", "res_norm", "res_norm_reg", "taps_res_norm_reg")}

# the DROP / RES instantiation families (BF: the bf16-storage flag, both values required), as regular expressions over the names above
N = r"\d+"
FAMILIES = {
    "edge_fwd3_kernel<.., BF, true>": (0, rf"edge_fwd3_kernel<{N}, {N}, {N}, BF, true>"),
    "edge_fwd2_kernel<.., BF, true>": (0, rf"edge_fwd2_kernel<{N}, {N}, {N}, BF, true>"),
    "edge_fwd_kernel<.., true, BF, true>": (0, rf"edge_fwd_kernel<{N}, {N}, true, BF, true>"),
    # records (false) or message rows (true): at the default settings an fp32 shape with a record path always keeps records, so the fp32
    # message-row form runs only under GAT_BWD_STASH=0 and is no row of this table; bf16 storage reaches both (records at H*D = 64)
    "edge_bwd3_kernel<.., BF, stash|msg, true>": (2, rf"edge_bwd3_kernel<{N}, {N}, {N}, 0, BF, (false|true), true>"),
    "edge_bwd2_kernel<.., BF, false, true>": (2, rf"edge_bwd2_kernel<{N}, {N}, {N}, 0, BF, false, true>"),
    "edge_bwd_kernel<.., true, true, 0, BF, true>": (2, rf"edge_bwd_kernel<{N}, {N}, true, true, 0, BF, true>"),
}


def test_coverage_table_is_the_matrix():
    assert len(COVERAGE) == 112
    assert sorted(COVERAGE) == sorted((hd, d, dt == "bf16", form) for hd, d, dt, form in T.CASES)
    assert len({T.case_id(c) for c in T.CASES}) == 112


def test_every_drop_family_appears_in_both_storage_modes():
    for name, (col, pat) in FAMILIES.items():
        for bf in ("false", "true"):
            rx = re.compile(pat.replace("BF", bf) + "$")
            hits = [k for k, v in COVERAGE.items() if rx.match(v[col])]
            assert hits, (name, bf)
            assert all(k[2] == (bf == "true") for k in hits)
    drop3 = {(m.group(1), m.group(2)) for v in COVERAGE.values()
             for m in [re.match(rf"edge_bwd3_kernel<{N}, {N}, {N}, 0, (\w+), (\w+), true>$", v[2])] if m}
    assert drop3 == {("false", "false"), ("true", "false"), ("true", "true")}      # (BF, message rows)
    for alpha in ("false", "true"):                                  # the RES fix-up of the split rows, without and with alpha
        hits = {(k[0], k[1]) for k, v in COVERAGE.items() if re.match(rf"edge_fwd_fix_kernel<{N}, {N}, {alpha}, true>$", v[1])}
        assert len(hits) == 14, alpha
    plain_fix = {(k[0], k[1]) for k, v in COVERAGE.items() if re.match(rf"edge_fwd_fix_kernel<{N}, {N}, false>$", v[1])}
    assert len(plain_fix) == 14


def test_every_shape_reaches_its_drop_forward_and_backward():
    for (hd, d) in T.SHAPES:
        for bf16 in (False, True):
            fwd = {COVERAGE[(hd, d, bf16, f)][0] for f in T.FORMS}
            bwd = {COVERAGE[(hd, d, bf16, f)][2] for f in T.FORMS}
            assert len(fwd) == 2 and all(k.endswith(", true>") for k in fwd)       # the packed DROP forward and the ALPHA one
            assert len(bwd) == 3                                                   # DROP backward, default backward, the tap form's
            assert all(f"<{hd}, {d}," in k for k in fwd | bwd)


def test_shapes_with_and_without_a_record_path_both_occur():
    with_n = [s for s in T.SHAPES if stash_n(*s)]
    assert sorted(with_n) == [(8, 4), (16, 4), (32, 4), (32, 8), (64, 4), (64, 8)] and len(with_n) < len(T.SHAPES)
    # rows per wave of the group-per-row kernels: 64 / (HD / N) — 4 at (64, 8), 16 at (8, 4)
    assert 64 // (64 // stash_n(64, 8)) == 4 and 64 // (8 // stash_n(8, 4)) == 16
    # records under bf16 storage only at H*D = 64
    assert COVERAGE[(64, 8, True, "reg")][2].endswith("true, false, true>") and COVERAGE[(32, 8, True, "reg")][2].endswith("true, true, true>")
    # a few rows spelled out, read off the selectors by hand
    assert COVERAGE[(64, 8, False, "res_norm_reg")] == ("edge_fwd3_kernel<64, 8, 4, false, true>", "edge_fwd_fix_kernel<64, 8, false, true>",
                                                        "edge_bwd3_kernel<64, 8, 4, 0, false, false, true>")
    assert COVERAGE[(32, 32, True, "reg")] == ("edge_fwd2_kernel<32, 32, 4, true, true>", "edge_fwd_fix_kernel<32, 32, false>",
                                               "edge_bwd2_kernel<32, 32, 4, 0, true, false, true>")
    assert COVERAGE[(16, 8, False, "res_norm")] == ("edge_fwd2_kernel<16, 8, 2, false, true>", "edge_fwd_fix_kernel<16, 8, false, true>",
                                                    "edge_bwd2_kernel<16, 8, 2, 0, false>")
    assert COVERAGE[(8, 4, True, "taps_res_norm_reg")] == ("edge_fwd_kernel<8, 4, true, true, true>", "edge_fwd_fix_kernel<8, 4, true, true>",
                                                           "edge_bwd_kernel<8, 4, true, true, 0, true, true>")


def test_the_graph_is_the_one_the_cases_need():
    g = parity_graph()
    assert g["n"] == 150 and g["n"] % 16 != 0 and len(g["col_idx"]) == 1000
    assert int(g["row_ptr"][8] - g["row_ptr"][7]) == 300 and g["row_ptr"][3] == g["row_ptr"][4]


@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("hd,d", T.SHAPES, ids=[f"hd{hd}_d{d}" for hd, d in T.SHAPES])
def test_some_of_the_first_40_seeds_is_clear_of_the_kink(orc, hd, d, dt):
    """pick_shape of tests/feature_cases.py raises when none of the first 40 seeds keeps the model off the kinks; the reference
    alone must offer one for each of the three models the four forms run (the keep_taps form shares res_norm_reg's)."""
    g, heads, outdims, cfg = T.shape_model(orc, hd, d)
    assert heads[0] * outdims[0] == hd
    for norm, reg in ((False, True), (True, False), (True, True)):
        T.pick_shape(orc, cfg, g, norm, REG if reg else None, dt == "bf16")


def _alpha_cases(orc, hd, d, reg):
    g, heads, outdims, cfg = T.shape_model(orc, hd, d)
    keeps, attn, feat = masks(cfg, g, cfg.heads, reg)
    P = orc.xavier_params(cfg, 1)
    ref = T.run_model(cfg, g, P, keeps=keeps, attn=attn, feat=feat)
    return g, cfg, P, keeps, ref


@pytest.mark.parametrize("reg", [None, REG], ids=["plain", "regularised"])
@pytest.mark.parametrize("hd,d", [(64, 8), (8, 4), (64, 64)])
def test_alpha_key_is_a_softmax_over_the_survivors(orc, hd, d, reg):
    g, cfg, P, keeps, ref = _alpha_cases(orc, hd, d, reg)
    E = len(g["col_idx"])
    dst = np.repeat(np.arange(g["n"]), np.diff(g["row_ptr"]))
    assert len(ref["alpha"]) == cfg.L
    for l in range(cfg.L):
        al = ref["alpha"][l]
        k = np.ones(E, bool) if keeps is None else np.asarray(keeps[l], bool)
        assert al.shape == (cfg.heads[l], E) and al.dtype == np.float64
        assert (al[:, ~k] == 0).all() and (al[:, k] > 0).all()
        sums = np.zeros((cfg.heads[l], g["n"]))
        for h in range(cfg.heads[l]):
            np.add.at(sums[h], dst, al[h])
        alive = np.bincount(dst[k], minlength=g["n"]) > 0
        assert alive.sum() > 100 and not alive[3]
        assert np.abs(sums[:, alive] - 1).max() <= 1e-12
        assert (sums[:, ~alive] == 0).all()
    if reg is not None:
        assert all(0 < np.asarray(k).sum() < E for k in keeps)


@pytest.mark.parametrize("hd,d", T.SHAPES, ids=[f"hd{hd}_d{d}" for hd, d in T.SHAPES])
def test_alpha_key_is_the_oracles_alpha(orc, hd, d):
    """No regulariser, no norm: the key against the alpha tap of the CPU oracle's step on the same inputs, at 1e-6."""
    g, cfg, P, _, ref = _alpha_cases(orc, hd, d, None)
    want = orc.step(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P)
    for l in range(cfg.L):
        a = np.asarray(want.taps["alpha"][l])
        assert a.shape == ref["alpha"][l].shape and np.abs(a).max() > 0
        assert np.abs(ref["alpha"][l] - a).max() <= 1e-6
