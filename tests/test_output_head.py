"""The output head of a context (gat_head.hip: head_forward_kernel<8|16|32|64|0>, head_step_kernel,
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


@pytest.mark.parametrize("DL", [4, 8, 16])
@pytest.mark.parametrize("C", [7, 47, 64])
def test_paths_agree_bitwise(pkg, C, DL):
    """The softmax head's two paths at the register-blocked shapes, on twin contexts: gat_step (head_step_kernel) against gat_forward +
    gat_backward (head_forward_kernel, head_backward2_kernel) — loss, #correct, grad_Wo and every other gradient group bitwise, and the
    y of a forward bitwise across the twins.  n = 129: one full 128-row tile and a ragged tile of one row.  The kernels share their
    pieces (gat_head.hip); this holds what they promise of each other.

    D_last = 16 under 8 heads is H * D = 128, outside the edge fast path: the generic edge backward adds into gPL with float atomics, so
    the groups behind it (W, a) do not reproduce from one run to the next, whatever the head does — measured on the library before the
    pieces were cut: grad_W of the twins differs at all three C by up to 2e-7 of its largest magnitude (profiles/head_pieces/README.md).
    At those three shapes the head's own outputs (loss, #correct, grad_Wo, y) are held bitwise and the other groups are not compared."""
    A = pkg.abi
    fast_edges = 8 * DL <= 64
    case = hc.Case(f"paths-C{C}-D{DL}", C, (8, DL), n=129)
    inp = hc.make_inputs(case)

    def twin():
        ctx = pkg.GatContext(case.heads, case.outdims, case.in_dim, C)
        ctx.set_graph(inp["rp"], inp["ci"]); ctx.set_features(inp["x"]); ctx.set_labels(inp["lab"])
        for grp, k in ((A.PARAM_W, "W"), (A.PARAM_A, "a"), (A.PARAM_WO, "Wo")):
            ctx.params_set(grp, inp[k])
        ctx.zero_grad()
        return ctx

    with twin() as st, twin() as fb:
        ls, cs = st.step()
        lf, cf = fb.forward()
        yf = fb.tap(A.TAP_Y)
        fb.backward()
        assert ls == lf and cs == cf, (ls, lf, cs, cf)
        assert st.grads_get(A.PARAM_WO).any()
        for k in A.PARAM_GROUPS:
            gs, gf = st.grads_get(k), fb.grads_get(k)
            if gs.size and not np.array_equal(gs, gf):
                print(f"group {k}: max |step - fwdbwd| = {np.abs(gs - gf).max():.3e} of max {np.abs(gf).max():.3e}")
            assert np.array_equal(gs, gf) or not (fast_edges or k == A.PARAM_WO), k
        assert st.forward() == (lf, cf)                     # the stepped context's own forward: y was never stored by its step
        ys = st.tap(A.TAP_Y)
        assert ys.shape == (129, C) and np.array_equal(ys, yf)


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
