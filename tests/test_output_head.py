"""The output head of a context (gat_dense_kernels.hip: head_forward_kernel<8|16|32|64|0>, head_step_kernel,
head_backward2_kernel, the generic head_backward_kernel, gat_eval_mask; head_rows_kernel and the fused last layer under
GAT_FUSE_LAST=1) isolated from everything upstream and held to the fp64 reference tests/head_ref.py: the procedure,
the tolerances and the case lists are in tests/head_cases.py.

Covered: num_classes across the fused / generic switch (64 | 65) and the switch of the incremental index walk
(256 | 257); every padded D_last width and the any-size fallback; node counts around the 128-node tile and one with more
tiles than blocks and a ragged last tile; gat_step, gat_forward + gat_backward, keep_taps, the flat LReLU' index, bf16
storage, a training mask; a saturated softmax (the 1e-12 clamp alone decides a node's loss); exact ties (first maximum
wins); both refusals.  Achieved errors are recorded with parity.record (tests/parity.py writes
them out at the end of the session) and copied to profiles/head_tests/.

Measured on the MI355X (profiles/head_tests/achieved_errors.json): see that file; every case passes at the bars above.
"""
import os
import textwrap

import numpy as np
import pytest

import head_cases as hc
import head_ref as hr
import parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", hc.CASES, ids=lambda c: c.name)
def test_head(pkg, case):
    hc.run_case(pkg, case)


def test_refusals(pkg):
    """num_classes * D_last > 2048: the backward / the step return GAT_E_UNSUPPORTED naming the output head, and a forward on
    the same context afterwards is still right; a Wo that leaves no room for a 32-node tile in LDS: the forward is refused."""
    A = pkg.abi
    case = hc.Case("refusal-C300", 300, (8, 8))
    assert case.refused
    inp = hc.make_inputs(case)
    with pkg.GatContext(case.heads, case.outdims, case.in_dim, case.C) as ctx:
        ctx.set_graph(inp["rp"], inp["ci"]); ctx.set_features(inp["x"]); ctx.set_labels(inp["lab"])
        for grp, k in ((A.PARAM_W, "W"), (A.PARAM_A, "a"), (A.PARAM_WO, "Wo")):
            ctx.params_set(grp, inp[k])
        ctx.zero_grad()
        for fn in (ctx.step, ctx.backward, ctx.head_backward):
            with pytest.raises(A.GatError) as ei:
                fn()
            assert ei.value.code == hc.GAT_E_UNSUPPORTED and "output head" in str(ei.value) and "2048" in str(ei.value)
        assert not ctx.grads_get(A.PARAM_WO).any()                  # a refused backward leaves nothing half-added
        loss, correct = ctx.forward()
        ref = hr.head_ref(ctx.tap(A.TAP_HOUT, 1), ctx.tap(A.TAP_HPRE, 1), inp["Wo"], inp["lab"], None, 8, hc.SLOPE)
        parity.check_abs("y", ctx.tap(A.TAP_Y), ref.y)
        err = abs(loss - ref.nll.sum()) / case.n
        parity.record("loss/n", err, parity.TOL)
        assert err <= parity.TOL
        assert len(ref.undecided) <= 2
        sure = int((np.delete(ref.pred == inp["lab"], ref.undecided)).sum())
        assert sure <= correct <= sure + len(ref.undecided)
    case = hc.Case("refusal-C400", 400, (1, 64), layers=1, in_dim=10)
    inp = hc.make_inputs(case)
    with pkg.GatContext(case.heads, case.outdims, case.in_dim, case.C) as ctx:
        ctx.set_graph(inp["rp"], inp["ci"]); ctx.set_features(inp["x"]); ctx.set_labels(inp["lab"])
        for grp, k in ((A.PARAM_W, "W"), (A.PARAM_A, "a"), (A.PARAM_WO, "Wo")):
            ctx.params_set(grp, inp[k])
        for fn in (ctx.forward, ctx.step):
            with pytest.raises(A.GatError) as ei:
                fn()
            assert ei.value.code == hc.GAT_E_UNSUPPORTED and "output head" in str(ei.value) and "LDS tile" in str(ei.value)


SNIPPET = """
    import sys
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import __graft_entry__ as entry
    import head_cases as hc, parity
    pkg = entry.load_package()
    for name in {names!r}:
        parity.set_test("tests/test_output_head.py::test_head_switches[{key}]/" + name)
        hc.run_case(pkg, hc.BY_NAME[name])
        print("OK", name, flush=True)
    parity.flush()
    print("ALL OK")
"""


@pytest.fixture(scope="module")
def children():
    """GAT_FUSE_LAST and GAT_HEAD_NODES are read once per process: one child per setting, in the child's environment only."""
    from conftest import run_snippets_parallel
    jobs = {}
    for key, (env, cases) in hc.CHILDREN.items():
        code = textwrap.dedent(SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), names=[c.name for c in cases], key=key))
        jobs[key] = (code, env)
    return run_snippets_parallel(jobs)


@pytest.mark.parametrize("key", list(hc.CHILDREN))
def test_head_switches(children, key):
    out = children[key]
    assert out.returncode == 0 and "ALL OK" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stdout.count("OK ") == len(hc.CHILDREN[key][1])
