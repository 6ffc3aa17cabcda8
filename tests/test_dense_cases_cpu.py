"""The dense case table (tests/dense_cases.py) checked without a GPU:
  * the cases and switch settings together reach EVERY kernel instantiation the dispatch macros of csrc/gat_gemm_kernels.hip can name
    (the list is read from the source text, the picks come from the Python restatement of the host rules — which the GPU test
    holds to the library's own report, case by case);
  * the bar has teeth: numpy models of wrong kernels fail it on the table's own inputs;
  * the honest model — six piece products per 16-k step, one fp32 rounding per MFMA, and the pessimistic one rounding per product —
    passes it."""
import os
import re

import numpy as np
import pytest

import dense_cases as DC
import dense_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "csrc", "gat_gemm_kernels.hip")

TABLE = [c for c in DC.CASES if not c["walk"]]
IDS = [c["id"] for c in TABLE]


def named_by_the_dispatch():
    txt = open(SRC).read()
    names = set()
    nts = re.findall(r"GAT_ROWGEMM_X3\((\d), W_, V_\)", txt)
    for w, v in re.findall(r"GAT_ROWGEMM_X3_NT\((\d), (true|false)\)", txt):
        names |= {f"rowgemm_x3_kernel<{nt}, {w}, {v}>" for nt in nts}
    names |= {f"rowgemm_pipe_kernel<{nt}>" for nt in re.findall(r"GAT_ROWGEMM_PIPE\((\d)\)", txt)}
    names |= {f"rowgemm_kernel<{nt}, {v}>" for nt, v in re.findall(r"GAT_ROWGEMM\((\d), (true|false)\)", txt)}
    for v, wm, bn in re.findall(r"GAT_GRADW\((true|false), (\d), (\d+)\)", txt):
        names |= {f"gradw_x3_kernel<{v}, {wm}, {bn}>", f"gradw_kernel<{v}, {wm}, {bn}>"}
    names |= set(re.findall(r"hipLaunchKernelGGL\(\(?(project_splitk(?:_x3)?_kernel<[^>]*>)", txt))
    return names


def test_cases_and_settings_reach_every_instantiation():
    named = named_by_the_dispatch()
    assert len(named) == 38, sorted(named)           # 12 x3 + 2 pipe + 6 fp32 row kernels, 12 grad_w, 6 split-K
    reached = {}
    for env, tag, _ in DC.SETTINGS:
        for c in DC.cases_of(tag):
            reached.setdefault(DC.pick(c, env), (tag, c["id"]))
    assert set(reached) <= named, sorted(set(reached) - named)
    assert not named - set(reached), f"no case reaches {sorted(named - set(reached))}"
    # every setting runs something, and something its switch changes
    for env, tag, _ in DC.SETTINGS[1:]:
        cs = DC.cases_of(tag)
        assert cs, tag
        if tag not in ("kmin=1024", "kmin=32", "cap=2"):       # (these change chunking and grids, not the kernel)
            assert any(DC.pick(c, env) != DC.pick(c, {}) for c in cs), tag


def test_case_table_respects_the_input_law():
    for c in DC.CASES:
        for name, (a, b) in DC.operands(c).items() if not c["walk"] else ():
            assert a.shape[0] * b.shape[0] <= 3000 * 128, (c["id"], name)
    # the special rows of hpre_prev: both zeros and the smallest denormals of either sign
    h = DC.inputs(next(c for c in DC.CASES if c["hpre"])["base"])["hpre"]
    assert h[0, 0] == 0 and not np.signbit(h[0, 0]) and np.signbit(h[1, 0]) and h[1, 0] == 0
    assert h[2, 0] > 0 and h[2, 0].view(np.int32) == 1 and h[3, 0] < 0


def _model(c, prod):
    return {name: DC.finish(c, name, prod(a, b)) for name, (a, b) in DC.operands(c).items()}


def _exact(a, b):
    return (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)


def _fails(c, outs):
    return bool(DC.judge(c, {}, outs)[1])


@pytest.mark.parametrize("c", TABLE, ids=IDS)
def test_wrong_kernels_fail_the_bar(c):
    ref = DC.reference(c)
    assert not _fails(c, _model(c, _exact)), "the correctly rounded product must pass"
    assert _fails(c, _model(c, R.bf16_once)), "operands rounded to bf16 once"
    assert _fails(c, _model(c, R.three_term)), "the three-term product"
    assert _fails(c, _model(c, R.dropped_last_step)), "a dropped last k-step"
    good = _model(c, _exact)
    if len(good) == 2:                                          # both halves: PL | PR, or the two halves of gradW
        l, r = sorted(good)
        assert _fails(c, {l: good[r], r: good[l]}), "left and right halves swapped"
        if c["kind"] == "grad_w":
            a, b = DC.operands(c)["R"]
            assert _fails(c, {"L": DC.finish(c, "L", _exact(a, b)), "R": np.zeros_like(good["R"])}), "the right half written into the left columns"
    if c["hpre"]:
        h = DC.inputs(c["base"])["hpre"]
        a, b = DC.operands(c)["gprev"]
        wrong = np.where(h >= 0, np.float32(1.0), np.float32(DC.SLOPE)).astype(np.float32)        # LReLU'(0) taken as 1
        assert _fails(c, {"gprev": (_exact(a, b) * wrong).astype(np.float32)}), "a missing LReLU' factor at hpre == 0"
        assert ref["gprev"]["factor"][0, 0] == np.float32(DC.SLOPE) and ref["gprev"]["factor"][2, 0] == 1


X3_ROWS = [c for c in TABLE if c["kind"] in ("project", "grad_x") and DC.pick(c, {}).startswith(("rowgemm_x3", "project_splitk_x3"))]


def _splitk_six_term(a, b):
    """the split-K projection: 128-wide chunks of K as six-term products, the slabs added in chunk order in fp32"""
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k0 in range(0, a.shape[1], 128):
        acc = (acc + R.six_term(a[:, k0:k0 + 128], b[:, k0:k0 + 128])).astype(np.float32)
    return acc


@pytest.mark.parametrize("c", X3_ROWS, ids=[c["id"] for c in X3_ROWS])
def test_the_honest_model_passes_the_bar(c):
    K = next(iter(DC.reference(c).values()))["K"]
    if DC.pick(c, {}).startswith("project_splitk"):
        assert not _fails(c, _model(c, _splitk_six_term))
        return
    recs, bad = DC.judge(c, {}, _model(c, R.six_term))
    assert not bad, bad
    if K <= 100:
        # The pessimistic model: a rounding after every one of the 6 K products, which no MFMA does (six times the roundings of the
        # fma chain).  It is held to the project's stated claim, 1e-6 * max(1, sqrt(K / 100)), up to K = 100; beyond, it sits at the
        # edge of it (K = 128).  On this table's draw it is NOT inside the chain-relative part everywhere: 9.78e-7 against 9.14e-7 at
        # K = 64 (200 x 64 x 32) and 9.15e-7 against 8.65e-7 at K = 50 (200 x 50 x 100) — the real kernels are held to both parts.
        recs, _ = DC.judge(c, {}, _model(c, lambda a, b: R.six_term(a, b, per_product=True)))
        for name, rec in recs.items():
            assert rec["ratio"] <= R.abs_bound(K), (c["id"], name, rec)
