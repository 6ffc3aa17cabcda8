"""Graph-level readout on the host (include/gatv2_abi.h "graph-level readout"): the fp64 model of tests/readout_ref.py against independent
formulations, the seed condition of every case tests/test_readout.py runs, the header and the ctypes declarations, the batch -> graph_ptr
conversion, and the train_edge refusals that end before any GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

import feature_cases as FC
import readout_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
HEADER = os.path.join(ROOT, "include", "gatv2_abi.h")
NEW_SYMBOLS = ["gat_set_readout", "gat_set_readout_device", "gat_readout_info", "gat_op_readout_forward", "gat_op_readout_backward"]


# -- the model
def rand_x(n=57, w=6, seed=0):
    import torch
    x = np.random.default_rng(seed).standard_normal((n, w))
    return torch.tensor(x, dtype=torch.float64, requires_grad=True), x


GP = np.array([0, 0, 1, 1, 20, 21, 57, 57])       # empty graphs in front, in the middle, behind; single rows; 19 and 36 rows


@pytest.mark.parametrize("mode", RR.MODES)
def test_pool_equals_scatter_formulations(mode):
    import torch
    X, x = rand_x()
    P, arg = RR.pool(X, GP, mode)
    G = len(GP) - 1
    idx = torch.from_numpy(RR.node_graph(GP)).long()[:, None].expand(-1, x.shape[1])
    red = {"sum": "sum", "mean": "mean", "max": "amax"}[mode]
    want = torch.zeros((G, x.shape[1]), dtype=torch.float64).scatter_reduce(0, idx, X.detach(), red, include_self=False)
    assert torch.allclose(P.detach(), want, rtol=0, atol=1e-14)
    cnt = np.diff(GP)
    assert np.all(P.detach().numpy()[cnt == 0] == 0) and np.all(arg[cnt == 0] == -1)      # the empty-graph rule
    if mode == "sum":
        assert torch.equal(P.detach(), torch.zeros((G, x.shape[1]), dtype=torch.float64).index_add(0, idx[:, 0], X.detach()))


@pytest.mark.parametrize("mode", RR.MODES)
def test_pool_gradient_is_the_closed_form(mode):
    import torch
    X, x = rand_x(seed=1)
    P, arg = RR.pool(X, GP, mode)
    gP = np.random.default_rng(2).standard_normal(P.shape)
    (P * torch.from_numpy(gP)).sum().backward()
    ng, cnt = RR.node_graph(GP), np.diff(GP)
    if mode == "sum":
        want = gP[ng]
    elif mode == "mean":
        want = gP[ng] / cnt[ng][:, None]
    else:
        want = np.where(arg[ng] == np.arange(len(ng))[:, None], gP[ng], 0.0)
        assert np.array_equal(arg[cnt > 0], np.stack([GP[g] + np.argmax(x[GP[g]:GP[g + 1]], axis=0) for g in np.flatnonzero(cnt > 0)]))
    np.testing.assert_allclose(X.grad.numpy(), want, rtol=0, atol=1e-15)


def test_max_takes_the_first_row_and_pool_gap():
    import torch
    x = np.array([[1.0, 5.0], [3.0, 5.0], [3.0, 2.0], [7.0, 7.0]])
    X = torch.tensor(x, requires_grad=True)
    gp = [0, 3, 4]
    P, arg = RR.pool(X, gp, "max")
    assert np.array_equal(arg, [[1, 0], [3, 3]]) and np.array_equal(P.detach().numpy(), [[3.0, 5.0], [7.0, 7.0]])
    P.sum().backward()
    assert np.array_equal(X.grad.numpy(), [[0, 1], [1, 0], [0, 0], [1, 1]])
    assert RR.pool_gap(x, gp, "max") == 0.0 and RR.pool_gap(x, gp, "mean") == np.inf
    assert RR.pool_gap(np.array([[1.0, 5.0], [3.0, 4.5], [9.0, 9.0]]), [0, 2, 3], "max") == 0.5      # single-row graphs do not count


def test_readout_of_one_node_graphs_is_the_node_model(orc):
    """graph_ptr = 0..N: every mode pools a row into itself, and the model is step_ref.forward with the same labels."""
    import step_ref as SR
    g = FC.host_graph(3)
    cfg = orc.Config([2, 2], [4, 4], g["f"], g["c"])
    P = orc.xavier_params(cfg, 1)
    base = SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P)
    base["loss"].backward()
    for mode in RR.MODES:
        ref = RR.forward(cfg, g, np.arange(g["n"] + 1), mode, g["labels"], P)
        ref["loss"].backward()
        assert abs(ref["loss"].item() - base["loss"].item()) < 1e-12
        for k in ("W", "a", "Wo"):
            np.testing.assert_allclose(ref[k].grad.numpy(), base[k].grad.numpy(), rtol=0, atol=1e-12)


def test_masked_graph_sends_no_gradient(orc):
    g = FC.host_graph(3)
    cfg = orc.Config([2, 2], [4, 4], g["f"], g["c"])
    P = orc.xavier_params(cfg, 1)
    gp = [0, 10, 10, 40]
    ref = RR.forward(cfg, g, gp, "mean", [0, 1, 2], P, gmask=[False, True, True])
    ref["loss"].backward()
    assert np.all(ref["pooled"].grad.numpy()[0] == 0) and np.abs(ref["pooled"].grad.numpy()[2]).max() > 0
    assert abs(ref["loss"].item() - ref["loss_per_graph"][1:].sum()) < 1e-12


# -- the seed condition of the GPU cases: a case without a clear seed fails HERE, never as a skip on the GPU
CASES = RR.cases(FC)


@pytest.mark.parametrize("case", CASES, ids=[RR.case_id(c) for c in CASES])
def test_every_gpu_case_has_a_clear_seed(orc, case):
    ci = RR.case_inputs(case)                            # raises when none of the 40 seeds is clear
    assert 0 <= ci["seed"] < 40
    ref = RR.forward(ci["cfg"], ci["g"], ci["graph_ptr"], ci["mode"], ci["glabels"], ci["P"], gmask=ci["gmask"], **ci["inp"], **ci["model_kw"])
    assert ref["s_min"] > 1e-5 and ref["y_label_min"] > RR.Y_MIN          # clear of the kinks and of the loss clamp
    ref["loss"].backward()
    assert RR.grads_min(ref) > RR.GRAD_MIN                                # every compared gradient has a scale
    if ci["mode"] == "max":
        assert ref["pool_gap"] > RR.GAP * ref["x_max"]
    else:
        assert ref["pool_gap"] == np.inf


ALL_BOUNDARY = RR.BOUNDARY + RR.BOUNDARY_SPARSE


@pytest.mark.parametrize("boundary", ALL_BOUNDARY, ids=[RR.boundary_id(b) for b in ALL_BOUNDARY])
def test_boundary_cases_have_a_clear_seed(orc, boundary):
    """The e2500 cases take their seed from behind the first 40 (tests/readout_ref.py BOUNDARY_SEEDS): the predicate is checked again here
    on the seed that was taken."""
    ci = RR.case_inputs(boundary=boundary)
    assert (0 <= ci["seed"] < 40 or ci["seed"] in RR.BOUNDARY_SEEDS) and max(np.diff(ci["graph_ptr"])) > 256      # longer than one segment
    ref = RR.model_of(ci)
    assert ref["s_min"] > 1e-5 and ref["hpre_min"] > 1e-5 and ref["y_label_min"] > RR.Y_MIN and RR.grads_min(ref) > RR.GRAD_MIN
    if ci["mode"] == "max":
        assert ref["pool_gap"] > RR.GAP * ref["x_max"]


def test_case_table():
    names = [c[0] for c in CASES]
    assert len(CASES) == 3 * (len(FC.FAMILIES) + 1) + 2 * 3 * 3 and "d5_scalar" in names
    assert RR.graph_mask(RR.GRAPH_PTR).tolist() == [True, True, True, True, False]


# -- header and bindings
def test_header_declares_the_feature():
    txt = open(HEADER).read()
    assert re.search(r"#define GAT_ABI_VERSION 6\b", txt)
    assert re.search(r"GAT_READOUT_NONE = 0, GAT_READOUT_MEAN = 1, GAT_READOUT_SUM = 2, GAT_READOUT_MAX = 3", txt)
    assert re.search(r"GAT_TAP_POOLED = 18\b", txt)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", txt), s


def test_abi_py_declares_the_feature(pkg):
    A = pkg.abi
    src = open(os.path.join(os.path.dirname(A.__file__), "abi.py")).read()
    for s in NEW_SYMBOLS:
        assert f'"{s}"' in src and s in A.declared_symbols(), s
    assert (A.READOUT_NONE, A.READOUT_MEAN, A.READOUT_SUM, A.READOUT_MAX, A.TAP_POOLED) == (0, 1, 2, 3, 18)
    assert [A.readout_mode(m) for m in ("mean", "sum", "max", "none", 3)] == [1, 2, 3, 0, 3]
    with pytest.raises(ValueError):
        A.readout_mode("median")
    for name in ("set_readout", "set_readout_device", "readout_info"):
        assert callable(getattr(A.GatContext, name))
    assert callable(A.op_readout_forward) and callable(A.op_readout_backward)


def test_batch_to_graph_ptr(pkg):
    A = pkg.abi
    assert A.batch_to_graph_ptr([0, 0, 1, 3, 3, 3]).tolist() == [0, 2, 3, 3, 6]       # id 2 does not occur: an empty graph
    assert A.batch_to_graph_ptr([2]).tolist() == [0, 0, 0, 1]
    assert A.batch_to_graph_ptr(RR.node_graph(RR.GRAPH_PTR)).tolist() == RR.GRAPH_PTR
    assert A.batch_to_graph_ptr(np.array([0, 1, 1])).dtype == np.int32
    for bad in ([0, 1, 0], [1, 0]):
        with pytest.raises(ValueError, match="sorted"):
            A.batch_to_graph_ptr(bad)
    with pytest.raises(ValueError):
        A.batch_to_graph_ptr([-1, 0])
    with pytest.raises(ValueError):
        A.batch_to_graph_ptr([])


def test_graph_batch_generator(pkg):
    S = pkg.synth
    a = S.graph_batch(50, 3, 9, 2.5, seed=4)
    b = S.graph_batch(50, 3, 9, 2.5, seed=4)
    for k in ("row_ptr", "col_idx", "graph_ptr", "x", "labels"):
        assert np.array_equal(a[k], b[k]), k                               # deterministic
    gp, rp, ci = a["graph_ptr"], a["row_ptr"], a["col_idx"]
    n = int(gp[-1])
    assert len(gp) == 51 and gp[0] == 0 and a["n"] == n and len(rp) == n + 1 and rp[-1] == len(ci) == a["e"]
    sizes = np.diff(gp)
    assert sizes.min() >= 3 and sizes.max() <= 9
    ng = RR.node_graph(gp)
    dst = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(ng[dst], ng[ci])                                 # block-diagonal: no edge leaves its graph
    for r in range(n):
        assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) >= 0)                   # sources ascending inside a row
    assert a["x"].shape == (n, a["f"]) and a["x"].dtype == np.float32
    assert a["labels"].shape == (50,) and a["labels"].min() >= 0 and a["labels"].max() == a["c"] - 1
    assert not np.array_equal(S.graph_batch(50, 3, 9, 2.5, seed=5)["col_idx"], ci)


# -- the host program: refused before any GPU call
def run(args):
    e = dict(os.environ)
    e.pop("DATA_ROOT", None)
    return subprocess.run([BIN] + args, capture_output=True, text=True, env=e, timeout=600)


def test_train_edge_readout_refusals(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    base = ["--heads", "8,8", "--outdims", "8,8", "--dataset", "mols", "--data-root", str(tmp_path)]
    (tmp_path / "mols").mkdir()
    for args, msg in ((base + ["--readout", "bogus"], "Error: --readout must be mean, sum or max\n"),
                      (base + ["--readout"], "Error: --readout must be mean, sum or max\n"),
                      (base + ["--readout", "mean"], f"Error: --readout needs graph_ptr.txt (G+1 integers: the first node of every graph, then "
                                                     f"the node count) in {tmp_path}/mols/\n"),
                      (base + ["--readout", "max", "--ranks", "2"],
                       "Error: --readout needs --ranks 1: a graph of the batch may straddle two destination-range shards\n")):
        r = run(args)
        assert r.returncode == 1 and r.stderr.endswith(msg), (args, r.stderr)
        assert "[Memory Tracker]" not in r.stdout and "Configuration:" not in r.stdout      # nothing touched the GPU
    assert "--readout mean|sum|max" in run(["--help"]).stdout
