"""Every branch of the dense dispatch (csrc/gat_gemm_kernels.hip: run_rowgemm, the split-K projection, grad_w's tile shapes, the
residual kernels' K chunks) and every dense switch, held to the fp64 product of the same fp32 operands through the stateless
gat_op_dense_* seams — one launcher per call, exact operands, guard bands around every buffer (tests/dense_cases.py has the table and
the harness, tests/dense_ref.py the bar).  For every (case, setting) the seam reports the kernel it launched, and that must be the one
the host rules name: a case proves that it reached its branch.

The default setting runs in this process, case by case; every setting (the default again) runs in a child of its own — the switches
are read once per process — which also asserts through gat_switches() that the library read its setting and nothing else.  Exact
checks: the bf16 epilogue against the fp32 launch, the LeakyReLU' decisions of grad_x, and the tile walk (GAT_RESIDENT_CAP=2 makes a
block walk several tiles: bit-identical outputs to the uncapped child's)."""
import json
import os
import textwrap

import numpy as np
import pytest

import dense_cases as DC
import dense_ref as R
import parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = [c for c in DC.cases_of("default") if not c["walk"]]

SNIPPET = """
    import sys
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import __graft_entry__ as entry
    import dense_cases as DC
    pkg = entry.load_package()
    try:
        n = DC.run_setting(pkg, {tag!r})
    finally:
        print("SWITCHES", pkg.abi.switches())
    print("OK cases", n)
"""


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def setting_runs():
    from conftest import run_snippets_parallel
    jobs = {tag: (textwrap.dedent(SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), tag=tag)), env) for env, tag, _ in DC.SETTINGS}
    return run_snippets_parallel(jobs, timeout=300)


def _results(out):
    return {r["id"]: r for r in (json.loads(line[7:]) for line in out.stdout.splitlines() if line.startswith("RESULT "))}


@pytest.mark.parametrize("c", DEFAULT, ids=[c["id"] for c in DEFAULT])
def test_default_kernels(pkg, torch, c):
    res = DC.run_case(pkg.abi, torch, c, {})
    DC.record_case(parity, c, "default", res)
    for name, rec in res["records"].items():
        print(f"{c['id']} {name}: {res['picked']} ratio {rec['ratio']:.3g} chain {rec['rc']:.3g} share {rec['share']:.2f}")
    assert not res["failures"], "\n".join(res["failures"])
    if c["kind"] == "grad_w" and c["M"] in (6273, 8300) and c["part"] == DC.BOTH:
        # 128-node chunks: 50 and 65 slabs, beyond the 48 at which reduce_slabs_kernel enters its four-way unrolled loop
        assert res["scratch_floats"] == -(-c["M"] // 128) * 2 * c["HD"] * c["F"], res["scratch_floats"]


@pytest.mark.parametrize("env,tag", [(e, t) for e, t, _ in DC.SETTINGS], ids=[t for _, t, _ in DC.SETTINGS])
def test_switch_settings(setting_runs, env, tag):
    out = setting_runs[tag]
    assert out.returncode == 0 and f"OK cases {len(DC.cases_of(tag))}" in out.stdout, (out.stdout[-3000:], out.stderr[-3000:])
    taken = dict(kv.split("=", 1) for kv in out.stdout.split("SWITCHES", 1)[1].splitlines()[0].split() if "=" in kv)
    assert taken == env, (taken, env)          # the setting was really taken, with these values, and nothing else steered the run
    res = _results(out)
    for c in DC.cases_of(tag):                 # (the child asserts the same; here it is visible per setting)
        assert res[c["id"]]["picked"] == DC.pick(c, env) and not res[c["id"]]["failures"], res[c["id"]]


def test_tile_walk_is_bit_identical(setting_runs):
    """A row's arithmetic does not depend on which block owns its tile: with at most two resident blocks every block of the 1100-row
    cases walks several tiles (the x3 kernel's ring keeps loads in flight across the boundary), and nothing may change."""
    capped, plain = _results(setting_runs["cap=2"]), _results(setting_runs["default"])
    walk = [c for c in DC.CASES if c["walk"]]
    assert len(walk) >= 30
    for c in walk:
        assert capped[c["id"]]["picked"] == plain[c["id"]]["picked"]
        assert capped[c["id"]]["sha"] == plain[c["id"]]["sha"], c["id"]


def test_refused_arguments_launch_nothing(pkg, torch):
    """Every refused argument gives GAT_E_INVALID before any launch: outputs and guard bands come back untouched."""
    A = pkg.abi
    M, F, HD = 40, 12, 8
    rng = np.random.default_rng(3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")      # noqa: E731
    x, W, g, Wres, h = dev(rng.standard_normal((M, F))), dev(rng.standard_normal((HD, 2 * F))), dev(rng.standard_normal((M, HD))), \
        dev(rng.standard_normal((HD, F))), dev(rng.standard_normal((M, F)))
    need = A.op_dense_scratch_floats(A.DENSE_SCRATCH_GRAD_W, M, F, HD)
    bufs = {k: R.Guarded(torch, n, np.full(n, 1.5, np.float32)) for k, n in
            (("pl", M * HD), ("pr", M * HD), ("gprev", M * F), ("gw", HD * 2 * F), ("scr", need), ("r", M * HD), ("gwres", HD * F), ("gx", M * F))}
    b = {k: v.ptr for k, v in bufs.items()}
    X, Wp, Gp, Wr = x.data_ptr(), W.data_ptr(), g.data_ptr(), Wres.data_ptr()
    refused = [
        lambda: A.op_dense_project(0, 0, Wp, M, F, HD, 0, False, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, 0, 0, M, F, HD, 0, False, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, 0, False, 0, b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, 0, False, b["pl"], 0),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, 1, False, 0, b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, 2, False, b["pl"], 0),
        lambda: A.op_dense_project(X, 0, Wp, -1, F, HD, 0, False, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, 0, HD, 0, False, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, F, 0, 0, False, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, F - 1, Wp, M, F, HD, 0, False, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, 3, False, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, -1, False, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, 0, 2, b["pl"], b["pr"]),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, 0, False, b["pl"], b["pr"], 0, 16),
        lambda: A.op_dense_project(X, 0, Wp, M, F, HD, 0, False, b["pl"], b["pr"], b["scr"], -1),
        lambda: A.op_dense_grad_x(0, Gp, Wp, 0, b["gprev"], M, F, HD, 0.2),
        lambda: A.op_dense_grad_x(Gp, 0, Wp, 0, b["gprev"], M, F, HD, 0.2),
        lambda: A.op_dense_grad_x(Gp, Gp, 0, 0, b["gprev"], M, F, HD, 0.2),
        lambda: A.op_dense_grad_x(Gp, Gp, Wp, h.data_ptr(), 0, M, F, HD, 0.2),
        lambda: A.op_dense_grad_x(Gp, Gp, Wp, 0, b["gprev"], -1, F, HD, 0.2),
        lambda: A.op_dense_grad_x(Gp, Gp, Wp, 0, b["gprev"], M, 0, HD, 0.2),
        lambda: A.op_dense_grad_x(Gp, Gp, Wp, 0, b["gprev"], M, F, 0, 0.2),
        lambda: A.op_dense_grad_x(Gp, Gp, Wp, 0, b["gprev"], M, F, HD, float("nan")),
        lambda: A.op_dense_grad_w(0, Gp, X, 0, b["gw"], b["scr"], need, M, F, HD, 0),
        lambda: A.op_dense_grad_w(Gp, 0, X, 0, b["gw"], b["scr"], need, M, F, HD, 0),
        lambda: A.op_dense_grad_w(0, Gp, X, 0, b["gw"], b["scr"], need, M, F, HD, 1),
        lambda: A.op_dense_grad_w(Gp, 0, X, 0, b["gw"], b["scr"], need, M, F, HD, 2),
        lambda: A.op_dense_grad_w(Gp, Gp, 0, 0, b["gw"], b["scr"], need, M, F, HD, 0),
        lambda: A.op_dense_grad_w(Gp, Gp, X, 0, 0, b["scr"], need, M, F, HD, 0),
        lambda: A.op_dense_grad_w(Gp, Gp, X, 0, b["gw"], 0, need, M, F, HD, 0),
        lambda: A.op_dense_grad_w(Gp, Gp, X, 0, b["gw"], b["scr"], need - 1, M, F, HD, 0),
        lambda: A.op_dense_grad_w(Gp, Gp, X, F - 1, b["gw"], b["scr"], need, M, F, HD, 0),
        lambda: A.op_dense_grad_w(Gp, Gp, X, 0, b["gw"], b["scr"], need, M, F, HD, 3),
        lambda: A.op_dense_grad_w(Gp, Gp, X, 0, b["gw"], b["scr"], need, -1, F, HD, 0),
        lambda: A.op_dense_grad_w(Gp, Gp, X, 0, b["gw"], b["scr"], need, M, 0, HD, 0),
        lambda: A.op_dense_grad_w(Gp, Gp, X, 0, b["gw"], b["scr"], need, M, F, 0, 0),
        lambda: A.op_dense_project_res(0, 0, Wr, b["r"], M, F, HD),
        lambda: A.op_dense_project_res(X, 0, 0, b["r"], M, F, HD),
        lambda: A.op_dense_project_res(X, 0, Wr, 0, M, F, HD),
        lambda: A.op_dense_project_res(X, F - 1, Wr, b["r"], M, F, HD),
        lambda: A.op_dense_project_res(X, 0, Wr, b["r"], -1, F, HD),
        lambda: A.op_dense_project_res(X, 0, Wr, b["r"], M, 0, HD),
        lambda: A.op_dense_project_res(X, 0, Wr, b["r"], M, F, 0),
        lambda: A.op_dense_grad_wres(0, X, 0, b["gwres"], b["scr"], need, M, F, HD),
        lambda: A.op_dense_grad_wres(Gp, 0, 0, b["gwres"], b["scr"], need, M, F, HD),
        lambda: A.op_dense_grad_wres(Gp, X, 0, 0, b["scr"], need, M, F, HD),
        lambda: A.op_dense_grad_wres(Gp, X, 0, b["gwres"], 0, need, M, F, HD),
        lambda: A.op_dense_grad_wres(Gp, X, 0, b["gwres"], b["scr"], need - 1, M, F, HD),
        lambda: A.op_dense_grad_wres(Gp, X, F - 1, b["gwres"], b["scr"], need, M, F, HD),
        lambda: A.op_dense_grad_wres(Gp, X, 0, b["gwres"], b["scr"], need, M, 0, HD),
        lambda: A.op_dense_grad_x_res(0, Wr, b["gx"], M, F, HD),
        lambda: A.op_dense_grad_x_res(Gp, 0, b["gx"], M, F, HD),
        lambda: A.op_dense_grad_x_res(Gp, Wr, 0, M, F, HD),
        lambda: A.op_dense_grad_x_res(Gp, Wr, b["gx"], -1, F, HD),
        lambda: A.op_dense_grad_x_res(Gp, Wr, b["gx"], M, F, 0),
        lambda: A.op_dense_scratch_floats(2, M, F, HD),
        lambda: A.op_dense_scratch_floats(0, M, F, HD, 5),
        lambda: A.op_dense_scratch_floats(1, -1, F, HD),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(A.GatError) as e:
            call()
        assert e.value.code == 10001 and "gat_op_dense_" in str(e.value), (i, str(e.value))
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert v.untouched(), f"a refused call wrote into {k}"
    # and the same buffers take a valid call: zero rows launch nothing and report no kernel
    assert A.op_dense_project(X, 0, Wp, 0, F, HD, 0, False, b["pl"], b["pr"]) == ""
    assert bufs["pl"].untouched() and bufs["pr"].untouched()


REDUCE_CODE = textwrap.dedent(f"""
    import sys, hashlib, numpy as np
    sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, "tests")!r})
    import __graft_entry__ as entry
    from conftest import small_graph
    pkg = entry.load_package(); orc = entry.load_oracle(); A = pkg.abi
    rng = np.random.default_rng(5)
    rp, ci = small_graph(rng, 260, 2600, hub=(9, 700), empty=(0, 3))
    x = rng.standard_normal((260, 12)).astype(np.float32)
    lab = rng.integers(0, 4, 260).astype(np.int32); lab[0] = 3
    cfg = orc.Config([8, 8], [8, 8], 12, 4)
    W, a, Wo = orc.xavier_params(cfg, 6)
    with pkg.GatContext([8, 8], [8, 8], 12, 4) as ctx:
        ctx.set_graph(rp, ci); ctx.set_features(x); ctx.set_labels(lab)
        for g, arr in enumerate((W, a, Wo)): ctx.params_set(g, arr)
        ctx.zero_grad(); loss, correct = ctx.step()
        for g, name in ((A.PARAM_W, "W"), (A.PARAM_A, "a"), (A.PARAM_WO, "Wo")):
            grad = np.ascontiguousarray(ctx.grads_get(g))
            assert np.all(np.isfinite(grad)) and np.abs(grad).max() > 0
            print("GRAD", name, hashlib.sha1(grad.tobytes()).hexdigest())
    print("SWITCHES", A.switches())
    print("OK")
""")


def test_reduce_batch_and_single_reductions_agree_bitwise():
    """reduce_batch_kernel (every slab reduction of a step in one launch) and reduce_slabs_kernel (GAT_REDUCE_BATCH=0: one launch each)
    are the same arithmetic in the same order: one step of the switch-matrix graph, every parameter gradient byte for byte."""
    from conftest import run_snippets_parallel
    runs = run_snippets_parallel({"batch": (REDUCE_CODE, {}), "single": (REDUCE_CODE, {"GAT_REDUCE_BATCH": "0"})}, timeout=300)
    grads = {}
    for k, out in runs.items():
        assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
        grads[k] = [line for line in out.stdout.splitlines() if line.startswith("GRAD ")]
        assert len(grads[k]) == 3
    assert "GAT_REDUCE_BATCH=0" in runs["single"].stdout.split("SWITCHES", 1)[1].splitlines()[0]
    assert "GAT_REDUCE_BATCH" not in runs["batch"].stdout.split("SWITCHES", 1)[1].splitlines()[0]
    assert grads["batch"] == grads["single"], (grads["batch"], grads["single"])
