"""The pair head on the host (include/gatv2_abi.h "pair head"): the fp64 model of tests/pair_ref.py against finite differences and the
closed-form adjoint, the seed condition of every case tests/test_pair_head.py runs, the header and the ctypes declarations, the pair
generator, and the train_edge refusals that end before any GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

import feature_cases as FC
import pair_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
HEADER = os.path.join(ROOT, "include", "gatv2_abi.h")
NEW_SYMBOLS = ["gat_set_pairs", "gat_set_pairs_device", "gat_pairs_info", "gat_op_pair_forward", "gat_op_pair_backward"]

# a u == v pair (3, 3), a duplicate pair (1, 4) twice, node 5 in no pair, node 0 as u and as v
U = np.array([0, 1, 3, 1, 2, 4, 1])
V = np.array([2, 4, 3, 4, 0, 0, 1])


# -- the model
@pytest.mark.parametrize("mode", PR.MODES)
def test_gather_gradient_is_the_closed_form_and_finite_differences(mode):
    import torch
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 5))
    gq = rng.standard_normal((len(U), 5))
    X = torch.tensor(x, requires_grad=True)
    Q = PR.gather(X, U, V, mode)
    assert np.array_equal(Q.detach().numpy(), x[U] * x[V] if mode == "mul" else x[U] + x[V])
    (Q * torch.from_numpy(gq)).sum().backward()
    want = np.zeros_like(x)                              # the header's formula: a sum over the incidences (p, role) of every node
    for p, (a, b) in enumerate(zip(U, V)):
        want[a] += gq[p] * (x[b] if mode == "mul" else 1.0)
        want[b] += gq[p] * (x[a] if mode == "mul" else 1.0)
    np.testing.assert_allclose(X.grad.numpy(), want, rtol=0, atol=1e-14)
    assert np.all(X.grad.numpy()[5] == 0)                # in no pair
    if mode == "mul":                                    # the u == v pair: d(x*x) = 2 x gQ, no special case
        lone = np.zeros_like(x)
        lone[3] = 2 * x[3] * gq[2]
        np.testing.assert_allclose(X.grad.numpy()[3], lone[3], rtol=0, atol=1e-14)

    def f(xx):
        q = xx[U] * xx[V] if mode == "mul" else xx[U] + xx[V]
        return float((q * gq).sum())
    h = 1e-6
    fd = np.zeros_like(x)
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            d = np.zeros_like(x); d[i, j] = h
            fd[i, j] = (f(x + d) - f(x - d)) / (2 * h)
    np.testing.assert_allclose(X.grad.numpy(), fd, rtol=0, atol=1e-8)


@pytest.mark.parametrize("loss", [PR.SOFTMAX, PR.BCE, PR.MSE])
@pytest.mark.parametrize("mode", PR.MODES)
def test_step_model_against_finite_differences(orc, mode, loss):
    """The whole model's gradient of Wo and of one slice of W, by central differences in fp64."""
    g = FC.host_graph(3)
    C = 1 if loss == PR.BCE else g["c"]
    g = dict(g, c=C)
    cfg = orc.Config([2, 2], [4, 4], g["f"], C)
    P = orc.xavier_params(cfg, 1)
    rng = np.random.default_rng(5)
    u = np.concatenate([U, rng.integers(0, g["n"], 20)]); v = np.concatenate([V, rng.integers(0, g["n"], 20)])
    n_pairs = len(u)
    if loss == PR.SOFTMAX:
        sup = rng.integers(0, C, n_pairs)
    elif loss == PR.BCE:
        sup = (rng.random((n_pairs, 1)) > 0.5).astype(np.float32)
    else:
        sup = rng.standard_normal((n_pairs, C)).astype(np.float32)
        sup[3, 1] = np.nan
    mask = rng.random(n_pairs) > 0.3
    ref = PR.forward(cfg, g, u, v, mode, loss, sup, P, mask=mask)
    ref["loss"].backward()

    def loss_at(W, Wo):
        return PR.forward(cfg, g, u, v, mode, loss, sup, (W, P[1], Wo), mask=mask)["loss"].item()
    h = 1e-5
    for name, idx in (("Wo", range(0, len(P[2]), 3)), ("W", range(0, len(P[0]), 37))):
        got = ref[name].grad.numpy()
        scale = np.abs(got).max()
        assert scale > 0
        for i in idx:
            Wp, Wm, Wop, Wom = (np.asarray(a, np.float64).copy() for a in (P[0], P[0], P[2], P[2]))
            if name == "Wo":
                Wop[i] += h; Wom[i] -= h
            else:
                Wp[i] += h; Wm[i] -= h
            fd = (loss_at(Wp, Wop) - loss_at(Wm, Wom)) / (2 * h)
            assert abs(fd - got[i]) <= 1e-6 * scale + 1e-9, (name, i, fd, got[i])
    # a pair outside the mask sends no gradient
    gQ = ref["paired"].grad.numpy()
    assert np.all(gQ[~mask] == 0) and np.abs(gQ[mask]).max() > 0
    if loss == PR.BCE and mode == "mul":
        # pair (3, 3) of the graph's empty row: Q == 0 exactly, z == 0, and dz = sigmoid(0) - t, not a subgradient of |z| or max(z, 0)
        assert np.all(ref["paired"].detach().numpy()[2] == 0) and mask[2]
        np.testing.assert_allclose(gQ[2], (0.5 - float(sup[2, 0])) * np.asarray(P[2], np.float64).reshape(-1), rtol=0, atol=1e-15)


# -- the seed condition of the GPU cases: a case without a clear seed fails HERE (none may be dropped), never as a skip on the GPU
CASES = PR.cases(FC)


@pytest.mark.parametrize("case", CASES, ids=[PR.case_id(c) for c in CASES])
def test_every_gpu_case_has_a_clear_seed(orc, case):
    ci = PR.case_inputs(case)                            # raises when none of the 40 seeds is clear
    assert 0 <= ci["seed"] < 40
    ref = PR.model_of(ci)
    assert ref["s_min"] > 1e-5
    if ci["loss"] == PR.SOFTMAX:
        assert ref["y_label_min"] > PR.Y_MIN
    for k in ("W", "a", "Wo"):
        assert float(ref[k].grad.abs().max()) > 0


def test_case_table_and_pair_list():
    names = [c[0] for c in CASES]
    assert len(CASES) == 2 * (len(FC.FAMILIES) + 1) + 2 * 2 * 2 + 2 * 3 * 2 and "d5_scalar" in names
    g = FC.parity_graph()
    u, v = PR.pair_list(g["n"])
    assert 380 <= len(u) <= 420 and u.min() >= 0 and max(u.max(), v.max()) < g["n"] - 1        # node n - 1 is in no pair
    inc = np.bincount(np.concatenate([u, v]), minlength=g["n"])
    assert inc[PR.HUB] > 256 and inc[g["n"] - 1] == 0                                          # segments + combine; a zero row
    assert np.any(u == v)
    pairs = list(zip(u.tolist(), v.tolist()))
    assert len(set(pairs)) < len(pairs)                                                        # a duplicate pair


# -- header and bindings
def test_header_declares_the_feature():
    txt = open(HEADER).read()
    assert re.search(r"#define GAT_ABI_VERSION 6\b", txt)
    assert re.search(r"GAT_PAIR_NONE = 0, GAT_PAIR_MUL = 1, GAT_PAIR_ADD = 2", txt)
    assert re.search(r"GAT_TAP_PAIRED = 19\b", txt)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", txt), s


def test_abi_py_declares_the_feature_and_the_library_exports_it(pkg):
    A = pkg.abi
    src = open(os.path.join(os.path.dirname(A.__file__), "abi.py")).read()
    lib = A.load_library()
    for s in NEW_SYMBOLS:
        assert f'"{s}"' in src and s in A.declared_symbols(), s
        assert getattr(lib, s) is not None, s            # exported by the built library
    assert (A.PAIR_NONE, A.PAIR_MUL, A.PAIR_ADD, A.TAP_PAIRED) == (0, 1, 2, 19)
    assert [A.pair_mode(m) for m in ("mul", "add", "none", 2)] == [1, 2, 0, 2]
    with pytest.raises(ValueError):
        A.pair_mode("concat")
    for name in ("set_pairs", "set_pairs_device", "pairs_info"):
        assert callable(getattr(A.GatContext, name))
    assert callable(A.op_pair_forward) and callable(A.op_pair_backward)
    assert isinstance(A.GatContext.head_rows, property)


def test_link_pairs_generator(pkg):
    S = pkg.synth
    ds = S.make_dataset("cora", scale=0.25)
    rp, ci, n = ds["row_ptr"], ds["col_idx"], ds["n"]
    a = S.link_pairs(rp, ci, 500, 300, seed=4)
    b = S.link_pairs(rp, ci, 500, 300, seed=4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                                        # deterministic
    u, v, t = a
    assert u.dtype == v.dtype == np.int32 and t.dtype == np.float32 and len(u) == len(v) == len(t) == 800
    assert u.min() >= 0 and v.min() >= 0 and u.max() < n and v.max() < n
    assert np.all(t[:500] == 1) and np.all(t[500:] == 0)
    for k in range(500):                                                   # every positive is an edge source -> destination of the graph
        assert u[k] in ci[rp[v[k]]:rp[v[k] + 1]]
    assert not np.array_equal(S.link_pairs(rp, ci, 500, 300, seed=5)[0], u)
    assert len(S.link_pairs(rp, ci, 0, 7, seed=1)[0]) == 7
    with pytest.raises(ValueError):
        S.link_pairs(rp, ci, -1, 3)


# -- the host program: refused before any GPU call
def run(args):
    e = dict(os.environ)
    e.pop("DATA_ROOT", None)
    return subprocess.run([BIN] + args, capture_output=True, text=True, env=e, timeout=600)


def test_train_edge_pairs_refusals(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    base = ["--heads", "8,8", "--outdims", "8,8", "--dataset", "links", "--data-root", str(tmp_path)]
    (tmp_path / "links").mkdir()
    for args, msg in ((base + ["--pairs", "concat"], "Error: --pairs must be mul or add\n"),
                      (base + ["--pairs"], "Error: --pairs must be mul or add\n"),
                      (base + ["--pairs", "mul"], f"Error: --pairs needs pairs.txt (one line \"u v\" per pair: two node indices) in {tmp_path}/links/\n"),
                      (base + ["--pairs", "add", "--ranks", "2"],
                       "Error: --pairs needs --ranks 1: an endpoint of a pair may live on another destination-range shard\n"),
                      (base + ["--pairs", "mul", "--readout", "mean"],
                       "Error: --pairs cannot be combined with --readout: the output head has one kind of row\n")):
        r = run(args)
        assert r.returncode == 1 and r.stderr.endswith(msg), (args, r.stderr)
        assert "[Memory Tracker]" not in r.stdout and "Configuration:" not in r.stdout      # nothing touched the GPU
    assert "--pairs mul|add" in run(["--help"]).stdout
