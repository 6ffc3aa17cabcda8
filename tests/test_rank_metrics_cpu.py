"""Ranking metrics without a GPU (include/gatv2_abi.h "ranking metrics"): the numpy reference of tests/rank_ref.py against an O(n^2)
pairwise brute force on every case the GPU seam test runs, and against sklearn where it is installed; the boundary (header, library
exports, the abi.py bindings, the struct's layout, the version); and the conditions tests/test_rank_metrics.py relies on, asserted on the
generated cases instead of assumed."""
import os
import re
import subprocess

import numpy as np
import pytest

import rank_cases as RC
import rank_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gatv2_abi.h")


@pytest.mark.parametrize("case", RC.seam_cases(), ids=RC.seam_ids())
def test_reference_is_the_pairwise_law(case):
    args = (case["scores"], case["labels"], case["targets"], case["mask"])
    want = RR.brute_force(*args, ks=RC.KS8)
    ks = RC.case_ks(case, int(want["n_neg"][0]))
    for k in (RC.KS8, ks):
        got = RR.rank_stats(*args, ks=k)
        RR.assert_same(got, RR.brute_force(*args, ks=k), (case["name"], k))
        for key in ("auc", "hits_at"):
            assert np.array_equal(got[key], RR.brute_force(*args, ks=k)[key], equal_nan=True), key
    if case["law"] == "equal":                           # one tie group: exactly half of every pair
        got = RR.rank_stats(*args)
        assert np.array_equal(got["auc_num"].astype(np.int64), got["n_pos"] * got["n_neg"])
    # Hits@K around the negative count: with K = n_neg + 1 (and K = n_neg when n_neg == 0) every positive counts
    got = RR.rank_stats(*args, ks=ks)
    assert got["hits"][0, 3] == got["n_pos"][0]


@pytest.mark.parametrize("case", RC.seam_cases(), ids=RC.seam_ids())
def test_reference_is_sklearn(case):
    M = pytest.importorskip("sklearn.metrics")
    got = RR.rank_stats(case["scores"], case["labels"], case["targets"], case["mask"])
    checked = 0
    for c in range(case["cols"]):
        s, pos, _ = RR.column_entries(case["scores"], case["labels"], case["targets"], case["mask"], c)
        if pos.all() or not pos.any():
            assert np.isnan(got["auc"][c])
            continue
        s = np.clip(s.astype(np.float64), -1e300, 1e300)                 # sklearn refuses +-inf: the order is what counts
        assert abs(got["auc"][c] - M.roc_auc_score(pos, s)) < 1e-12, (case["name"], c)
        assert abs(got["ap"][c] - M.average_precision_score(pos, s)) < 1e-12, (case["name"], c)
        checked += 1
    assert checked > 0 or case["rows"] <= 2 or case["cols"] == 1 or case["degenerate"]


def test_conditions_the_gpu_seam_tests_rely_on():
    cases = RC.seam_cases()
    assert {(c["rows"], c["cols"]) for c in cases} >= {(r, k) for r in RC.ROWS for k in RC.COLS}
    assert {c["law"] for c in cases} == set(RC.LAWS) and {c["kind"] for c in cases} == set(RC.INPUTS)
    assert any(c["mask"] is None for c in cases) and any(c["mask"] is not None for c in cases)
    assert any(c["stride"] > c["cols"] for c in cases) and any(c["stride"] == c["cols"] for c in cases)
    tie_heavy = [c for c in cases if c["tie_heavy"]]
    saturated = [c for c in cases if c["saturated"] and c["rows"] >= 1000]
    assert {c["cols"] for c in tie_heavy} == set(RC.COLS) and len(saturated) >= 2
    for case in cases:
        st = RR.rank_stats(case["scores"], case["labels"], case["targets"], case["mask"])
        both = (st["n_pos"] > 0) & (st["n_neg"] > 0)
        if case["rows"] >= 255 and case["kind"] != "labels" and not case["degenerate"]:
            assert both.all(), case["name"]              # every column has both classes
        if case["tie_heavy"] or case["saturated"]:
            for c in range(case["cols"]):
                s, pos, _ = RR.column_entries(case["scores"], case["labels"], case["targets"], case["mask"], c)
                vals, cnt = np.unique(s, return_counts=True)
                if case["saturated"]:
                    assert len(vals) <= 1 and cnt.sum() == len(s), case["name"]    # one group covering the whole column
                    assert len(s) > 256 or case["rows"] < 1000, case["name"]
                if case["tie_heavy"]:
                    big = [v for v, k in zip(vals, cnt) if k > 256 and pos[s == v].any() and not pos[s == v].all()]
                    assert big, (case["name"], c)        # a tie group of more than 256 entries holding both classes
        if case["degenerate"]:
            assert st["n_pos"][0] == 0 and st["n_neg"][0] > 0 and st["n_neg"][1] == 0 and st["n_pos"][1] > 0
            assert st["ap"][0] == 0.0 and st["mrr"][0] == 0.0 and np.isnan(st["auc"][0]) and np.isnan(st["auc"][1])
        if case["specials"]:
            s = case["scores"]
            assert np.isnan(s).any() and np.isinf(s).any() and (s == 0).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
            tiny = np.abs(s[(s != 0) & np.isfinite(s)]).min()
            assert 0 < tiny < np.finfo(np.float32).tiny and st["n_nan"].sum() > 0
            # -0.0 and +0.0 tie: folding them changes nothing
            folded = RR.rank_stats(np.where(s == 0, np.float32(0.0), s), case["labels"], case["targets"], case["mask"])
            RR.assert_same(st, folded, case["name"])


@pytest.mark.parametrize("name", RC.CONTEXTS)
def test_conditions_the_gpu_context_tests_rely_on(name):
    """P and N of a column depend on the supervision and the mask alone (a NaN score apart): at least C - 1 columns of every context case
    have both classes, whatever the device computes."""
    cc = RC.context_case(name)
    zeros = np.zeros((cc["rows"], cc["C"]), np.float32)
    st = RR.rank_stats(zeros, cc["labels"], cc["targets"], cc["mask"])
    both = (st["n_pos"] > 0) & (st["n_neg"] > 0)
    assert both.sum() >= max(cc["C"] - 1, 1), (name, st["n_pos"], st["n_neg"])
    assert 0 < cc["mask"].sum() < cc["rows"]
    if name == "node_bce_nan":
        assert np.isnan(cc["targets"]).any()
    if name == "pair_bce":
        assert cc["targets"][:RC.N_POS].all() and not cc["targets"][RC.N_POS:].any()


# -- the boundary
def test_header_declares_the_boundary():
    txt = open(HEADER).read()
    assert re.search(r"#define\s+GAT_ABI_VERSION\s+6\b", txt)
    assert re.search(r"#define\s+GAT_RANK_MAX_KS\s+8\b", txt)
    assert "ranking metrics" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    st = re.search(r"typedef\s+struct\s+gat_rank_stats\s*\{(.*?)\}\s*gat_rank_stats\s*;", code, flags=re.S)
    assert st, "struct gat_rank_stats"
    body = " ".join(st.group(1).split())
    assert body == "int64_t n_pos, n_neg, n_nan; uint64_t auc_num; double ap, mrr; int64_t hits[GAT_RANK_MAX_KS];", body
    flat = " ".join(code.split())
    assert ("int gat_eval_rank(gat_ctx* ctx, const uint8_t* mask, int64_t n_rows, const int32_t* ks, int32_t n_ks, gat_rank_stats* out );" in flat
            or "int gat_eval_rank(gat_ctx* ctx, const uint8_t* mask, int64_t n_rows, const int32_t* ks, int32_t n_ks, gat_rank_stats* out);" in flat)
    assert ("int gat_op_rank_stats(const float* d_scores, int64_t score_stride, const int32_t* d_labels, const float* d_targets, "
            "const uint8_t* d_mask, int64_t n_rows, int32_t n_cols, const int32_t* ks, int32_t n_ks, gat_rank_stats* out , void* stream);" in flat
            or "int32_t n_ks, gat_rank_stats* out, void* stream);" in flat)


def test_library_exports_and_bindings(pkg):
    A = pkg.abi
    new = {"gat_eval_rank", "gat_op_rank_stats", "gat_step_graph_state"}        # the last: how the tests see that a replay was not re-armed
    assert new <= set(A.declared_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert new <= exported
    assert callable(A.GatContext.step_graph_state)
    lib = A.load_library()
    assert lib.gat_abi_version() == 6
    assert len(lib.gat_eval_rank.argtypes) == 6 and len(lib.gat_op_rank_stats.argtypes) == 11
    assert callable(A.GatContext.eval_rank) and callable(A.op_rank_stats)
    assert A.RANK_MAX_KS == 8 and A.RANK_STATS_DTYPE.itemsize == 8 * (6 + A.RANK_MAX_KS)
    assert [A.RANK_STATS_DTYPE.fields[f][1] for f in ("n_pos", "n_neg", "n_nan", "auc_num", "ap", "mrr", "hits")] == [0, 8, 16, 24, 32, 40, 48]


def test_seam_checks_its_arguments_before_any_launch(pkg):
    """Every refusal of gat_op_rank_stats comes before anything touches a device (this test has none)."""
    A = pkg.abi
    E_INVALID, E_UNSUPPORTED = 10001, 10004

    def refused(code, text, **kw):
        args = dict(d_scores=64, score_stride=3, n_rows=4, n_cols=3, d_labels=64)
        args.update(kw)
        with pytest.raises(A.GatError) as ei:
            A.op_rank_stats(**args)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)

    refused(E_INVALID, "n_ks", ks=range(1, 10))
    refused(E_INVALID, "K must be >= 1", ks=(3, 0))
    refused(E_INVALID, "K must be >= 1", ks=(-1,))
    refused(E_INVALID, "n_cols < 1", n_cols=0)
    refused(E_INVALID, "n_rows < 0", n_rows=-1)
    refused(E_INVALID, "null", d_scores=0)
    refused(E_INVALID, "exactly one", d_targets=64)
    refused(E_INVALID, "exactly one", d_labels=0)
    refused(E_INVALID, "score_stride", score_stride=2)
    refused(E_UNSUPPORTED, "2^31", n_rows=2 ** 31 // 3 + 1)
    refused(E_UNSUPPORTED, "2^31", n_rows=2 ** 31, n_cols=1, score_stride=1)
    refused(E_UNSUPPORTED, "2^31", n_rows=2 ** 62, n_cols=4, score_stride=4)          # the product leaves 64 bits: still refused
    refused(E_UNSUPPORTED, "2^31", n_rows=2 ** 63 - 1, n_cols=47, score_stride=47)


def test_abi_dict_derives_the_ratios(pkg):
    A = pkg.abi
    out = np.zeros(3, A.RANK_STATS_DTYPE)
    out["n_pos"] = [2, 0, 4]; out["n_neg"] = [3, 5, 0]; out["auc_num"] = [9, 0, 0]; out["hits"][:, 0] = [1, 0, 4]; out["hits"][:, 1] = [2, 0, 4]
    d = A.rank_stats_dict(out, 2)
    assert d["hits"].shape == (3, 2) and d["auc"][0] == 0.75 and np.isnan(d["auc"][1]) and np.isnan(d["auc"][2])
    assert np.array_equal(d["hits_at"], [[0.5, 1.0], [np.nan, np.nan], [1.0, 1.0]], equal_nan=True)
