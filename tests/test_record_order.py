"""Edge-ordered records (GAT_STASH_ORDER): the fp32 record backward writes record j for CSR edge j and the wave-per-list pull pass fetches
it through the slot-to-edge index, instead of scattering the records to their source-major slots.  Each source's slots are summed in the
same order from the same words, so GAT_STASH_ORDER=0 and =1 must give BYTE-identical losses, parameter gradients and gPL tables (the
table behind every layer's layer_backward_edges, read through the phase API) — no tolerance.  The switch is a per-process static: one
child process per (case, setting), five at a time (conftest.run_snippets_parallel).

The graph (2 layers, heads (8, 8), outdims (8, 8), F = 16, C = 7, 300 rows, about 3,000 edges) holds a destination row of 600 in-edges
(split segments, the fix-up kernels), a source in every second row (150 slots: with GAT_GPL_HEAVY=16 the chunk kernel, as for every other
list beyond 16 slots), rows without in-edges, sources without out-edges, and an edge count that is no multiple of 16.

Where the rule refuses the layout (records_take_edge_order: the slot-parallel pull forced, bf16 storage) both settings must run the
scattered layout: they agree, and the library never reads the switch (gat_switches() does not list it)."""
import os
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = """
    import os, sys, numpy as np, torch
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import __graft_entry__ as entry
    from test_record_order import order_graph
    pkg = entry.load_package(); A = pkg.abi
    opt = {opt!r}
    g = order_graph()
    dev = torch.device("cuda", 0)
    ctx = pkg.GatContext([8, 8], [8, 8], 16, 7, dtype=opt.get("dtype", "f32"))
    if opt.get("edge_dim"):
        ctx.set_edge_dim(opt["edge_dim"])
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"]); ctx.set_labels(g["labels"])
    if opt.get("edge_dim"):
        ctx.set_edge_features(g["ea"][:, :opt["edge_dim"]])
    if opt.get("drop"):
        ctx.set_dropout(feat_p=0.0, attn_p=0.3, seed=5)
        ctx.set_dropedge(0.2)
    ctx.params_init(42)
    gpl = torch.zeros(300 * 64, device=dev)
    ctx.bind_table(A.TABLE_GPL, 0, gpl.data_ptr(), gpl.numel() * 4)
    groups = [k for k in A.PARAM_GROUPS if ctx.param_count(k) > 0]
    out = {{}}
    ctx.zero_grad()
    loss, correct = ctx.step()
    out["step_result"] = np.array([loss, correct], np.float64)
    for k in groups:
        out["step_grad%d" % k] = ctx.grads_get(k)
    ctx.zero_grad()
    for l in range(2):
        ctx.layer_project(l); ctx.layer_forward_edges(l)
    loss, correct = ctx.head_forward()
    out["phase_result"] = np.array([loss, correct], np.float64)
    ctx.head_backward()
    for l in (1, 0):
        ctx.layer_backward_edges(l)
        ctx.sync()
        out["gpl%d" % l] = gpl.cpu().numpy().copy()
        ctx.layer_backward_dense(l)
    ctx.sync()
    for k in groups:
        out["phase_grad%d" % k] = ctx.grads_get(k)
    ctx.close()
    np.savez(os.environ["RECORD_ORDER_OUT"], **out)
    print("SWITCHES<" + A.switches() + ">")
    print("OK")
"""


def order_graph():
    """The graph of this module (see the module text); drawn once per process, the children draw the same one."""
    rng = np.random.default_rng(20)
    n, n_src = 300, 280                              # sources 280 .. 299 have no out-edges
    rows = []
    for i in range(n):
        if i in (1, 2, 50):                          # rows without in-edges
            rows.append(np.zeros(0, np.int64))
            continue
        k = 600 if i == 7 else int(rng.integers(1, 15))
        r = rng.integers(0, n_src, k)
        if i % 2 == 0:
            r = np.concatenate([r, [5]])             # source 5: a slot list of about 150
        rows.append(np.sort(r))
    if sum(len(r) for r in rows) % 16 == 0:
        rows[9] = np.sort(np.concatenate([rows[9], [11]]))
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col_idx = np.concatenate(rows).astype(np.int32)
    e = int(row_ptr[-1])
    return dict(row_ptr=row_ptr, col_idx=col_idx, x=rng.standard_normal((n, 16)).astype(np.float32),
                labels=rng.integers(0, 7, n).astype(np.int32), ea=rng.standard_normal((e, 3)).astype(np.float32))


HEAVY = {"GAT_GPL_HEAVY": "16"}
# tag -> (environment beside the layout switch, context options, the rule gives the edge-ordered layout)
CASES = {
    "pull_last=0": (dict(HEAVY, GAT_PULL_LAST="0"), {}, True),
    "pull_last=1": (dict(HEAVY, GAT_PULL_LAST="1"), {}, True),
    "pull_last=0 v2=0": (dict(HEAVY, GAT_PULL_LAST="0", GAT_PULL_V2="0"), {}, True),
    "pull_last=1 v2=0": (dict(HEAVY, GAT_PULL_LAST="1", GAT_PULL_V2="0"), {}, True),
    "pull_last=0 v2=2": (dict(HEAVY, GAT_PULL_LAST="0", GAT_PULL_V2="2"), {}, True),
    "pull_last=1 v2=1": (dict(HEAVY, GAT_PULL_LAST="1", GAT_PULL_V2="1"), {}, True),
    "dropout dropedge": (dict(HEAVY, GAT_PULL_LAST="1"), {"drop": True}, True),
    "edge features": (dict(HEAVY), {"edge_dim": 3}, True),
    # four dword stores per lane and step in the place of the transposed 16-byte one (plain, DROP and PE instantiations)
    "lines=0": (dict(HEAVY, GAT_PULL_LAST="1", GAT_STASH_LINES="0"), {}, True),
    "lines=0 dropout dropedge": (dict(HEAVY, GAT_PULL_LAST="1", GAT_STASH_LINES="0"), {"drop": True}, True),
    "lines=0 edge features": (dict(HEAVY, GAT_STASH_LINES="0"), {"edge_dim": 3}, True),
    "refused: slot-parallel pull": (dict(HEAVY, GAT_PULL_RUNS="1"), {}, False),
    "refused: bf16 storage": (dict(HEAVY), {"dtype": "bf16"}, False),
}


def test_the_graph_has_what_the_cases_need():
    g = order_graph()
    rp, ci = g["row_ptr"], g["col_idx"]
    deg_in, deg_out = np.diff(rp), np.bincount(ci, minlength=300)
    assert len(rp) == 301 and 2500 <= rp[-1] <= 3500 and rp[-1] % 16 != 0
    assert deg_in.max() >= 600 and (deg_in == 0).sum() >= 3            # a split row (segments of 256 edges); empty rows
    assert deg_out.max() > 100 and (deg_out > 16).sum() >= 2 and (deg_out == 0).sum() >= 20      # chunked lists (several chunks and two); sources without slots


@pytest.fixture(scope="module")
def order_runs(tmp_path_factory):
    from conftest import run_snippets_parallel
    d = tmp_path_factory.mktemp("record_order")
    jobs = {}
    for tag, (env, opt, _) in CASES.items():
        for order in "01":
            code = textwrap.dedent(SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), opt=opt))
            f = str(d / f"{len(jobs)}.npz")
            jobs[(tag, order)] = (code, dict(env, GAT_STASH_ORDER=order, RECORD_ORDER_OUT=f))      # the child writes its arrays there
    return run_snippets_parallel(jobs, timeout=300), {k: e["RECORD_ORDER_OUT"] for k, (_, e) in jobs.items()}


@pytest.mark.parametrize("tag", list(CASES))
def test_edge_order_is_bitwise_the_scattered_layout(order_runs, tag):
    runs, files = order_runs
    env, _, allowed = CASES[tag]
    res = []
    for order in "01":
        out = runs[(tag, order)]
        assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
        taken = out.stdout.split("SWITCHES<", 1)[1].split(">", 1)[0].split()
        for k, v in env.items():                     # every setting was taken (GAT_STASH_LINES is read with edge order only)
            assert (f"{k}={v}" in taken) == (k != "GAT_STASH_LINES" or order == "1"), (k, v, taken)
        # the rule reads the layout switch only where the edge-ordered form exists: listed <=> the setting steered the run
        assert (f"GAT_STASH_ORDER={order}" in taken) == allowed, taken
        res.append(np.load(files[(tag, order)]))
    a, b = res
    assert sorted(a.files) == sorted(b.files) and {"gpl0", "gpl1", "step_result", "phase_result"} <= set(a.files)
    for key in a.files:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape
        assert np.isfinite(a[key]).all(), key
        assert a[key].tobytes() == b[key].tobytes(), (key, float(np.abs(a[key].astype(np.float64) - b[key].astype(np.float64)).max()))
    assert np.abs(a["gpl0"]).max() > 0 and np.abs(a["gpl1"]).max() > 0 and any(np.abs(a[k]).max() > 0 for k in a.files if "grad" in k)
