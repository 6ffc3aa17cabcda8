"""The hidden layer in front of the output head on the host (include/gatv2_abi.h "hidden layer"): the fp64 model of
tests/head_mlp_ref.py against finite differences, the seed condition of every case tests/test_head_mlp.py runs, the header, the ctypes
declarations and the library's exports, and the train_edge refusals and help text that end before any GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

import feature_cases as FC
import head_mlp_ref as HM
import head_model as HD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
HEADER = os.path.join(ROOT, "include", "gatv2_abi.h")
NEW_SYMBOLS = ["gat_set_head_hidden", "gat_head_hidden_info", "gat_op_head_hidden_forward", "gat_op_head_hidden_backward"]


# -- the model
@pytest.mark.parametrize("loss", [HM.SOFTMAX, HM.BCE, HM.MSE])
@pytest.mark.parametrize("kind", HM.KINDS)
def test_model_against_finite_differences(orc, kind, loss):
    """gradW1, gradb1, gradWo and a slice of gradW of the whole model by central differences in fp64, both activations in turn."""
    g = FC.host_graph(3)
    C = 1 if loss == HM.BCE else g["c"]
    g = dict(g, c=C)
    cfg = orc.Config([2, 2], [4, 4], g["f"], C)
    P = orc.xavier_params(cfg, 1)
    rng = np.random.default_rng(5)
    n = g["n"]
    graph_ptr = [0, 0, 1, 17, n] if kind == "readout" else None          # an empty graph, a single-node graph
    u = v = None
    if kind.startswith("pair"):
        u = np.concatenate([[0, 1, 3, 1], rng.integers(0, n, 20)]); v = np.concatenate([[2, 4, 3, 4], rng.integers(0, n, 20)])
    R = len(u) if u is not None else len(graph_ptr) - 1 if graph_ptr else n
    if loss == HM.SOFTMAX:
        sup = rng.integers(0, C, R)
    elif loss == HM.BCE:
        sup = (rng.random((R, 1)) > 0.5).astype(np.float32)
    else:
        sup = rng.standard_normal((R, C)).astype(np.float32)
        sup[min(3, R - 1), 1] = np.nan
    mask = rng.random(R) > 0.3
    mask[0] = True
    dh = 6
    W1, b1, Wo = (a.astype(np.float64) for a in HM.head_values(4, dh, C))
    act = "lrelu" if kind in ("node", "pair_add") else "relu"

    # float32-representable test values (forward() rounds its leaves to fp32), perturbed in fp64 below through a model of its own
    import torch

    def loss_at(W, W1_, b1_, Wo_):
        out = HM.forward(cfg, g, kind, loss, sup, (W, P[1]), np.zeros_like(W1), np.zeros_like(b1), np.zeros_like(Wo), act, mask=mask,
                         graph_ptr=graph_ptr, u=u, v=v)
        A = out["xin"] @ torch.from_numpy(W1_).t()
        z = HD.act(A + torch.from_numpy(b1_), act) @ torch.from_numpy(Wo_).t()
        return HD.loss(z, loss, sup, mask, detach_max=False, smooth_bce=True)[0].item()

    ref = HM.forward(cfg, g, kind, loss, sup, P[:2], W1, b1, Wo, act, mask=mask, graph_ptr=graph_ptr, u=u, v=v)
    assert HM.nonzero_min(ref["pre"]) > 1e-4                             # the differences do not step over a kink
    ref["loss"].backward()
    assert abs(loss_at(np.asarray(P[0], np.float64), W1, b1, Wo) - ref["loss"].item()) <= 1e-12 * max(1.0, abs(ref["loss"].item()))
    h = 1e-5
    for name, base, idx in (("W1", W1, range(0, W1.size, 2)), ("b1", b1, range(b1.size)), ("Wo", Wo, range(0, Wo.size, 2)),
                            ("W", np.asarray(P[0], np.float64), range(0, len(P[0]), 37))):
        got = ref[name].grad.numpy().reshape(-1)
        assert np.abs(got).max() > 0, name
        for i in idx:
            args = dict(W=np.asarray(P[0], np.float64), W1=W1, b1=b1, Wo=Wo)
            up, dn = base.copy().reshape(-1), base.copy().reshape(-1)
            up[i] += h; dn[i] -= h
            fd = (_call(loss_at, args, name, up.reshape(base.shape)) - _call(loss_at, args, name, dn.reshape(base.shape))) / (2 * h)
            np.testing.assert_allclose(fd, got[i], rtol=0, atol=1e-8, err_msg=f"{name}[{i}]")
    # a row outside the mask sends no gradient; the gradient reaches the rows the head read
    gz = ref["z1"].grad.numpy()
    assert np.all(gz[~mask] == 0) and np.abs(gz[mask]).max() > 0
    assert np.abs(ref["xin"].grad.numpy()).max() > 0


def _call(fn, args, name, value):
    a = dict(args)
    a[name] = value
    return fn(a["W"], a["W1"], a["b1"], a["Wo"])


def test_activation_convention_at_zero():
    """Z1 == 0 takes the slope branch in the backward: 0 for ReLU, the slope for LeakyReLU (torch's convention, the header's)."""
    import torch
    for name, want in (("relu", 0.0), ("lrelu", HD.SLOPE)):
        t = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        HD.act(t, name).sum().backward()
        assert np.all(t.grad.numpy() == want)


# -- the seed condition of the GPU cases: a case without a clear seed fails HERE (none may be dropped), never as a skip on the GPU
CASES = HM.cases()


@pytest.mark.parametrize("case", CASES, ids=[HM.case_id(c) for c in CASES])
def test_every_gpu_case_has_a_clear_seed(orc, case):
    ci = HM.case_inputs(case)                            # raises when none of the 40 seeds is clear
    assert 0 <= ci["seed"] < 40
    ref = HM.model_of(ci)
    assert ref["s_min"] > 1e-5
    assert float(np.abs(ref["pre"]).min()) > HM.A_MIN    # every |A + b1|: no decision of the stage sits on its kink
    assert HM.head_clear(ref, ci["loss"], ci["sup"], ci["mask"])
    for k in ("W", "a", "Wo", "W1", "b1"):
        assert float(ref[k].grad.abs().max()) > 0, k
    assert ref["z1"].shape == (ci["rows"], ci["dh"])


def test_case_table():
    fams = {c[0] for c in CASES}
    assert {"records_d8", "generic", "d5_scalar", "keep_taps", "bf16"} <= fams
    assert {c[2] for c in CASES} == set(HM.KINDS)
    assert {c[4] for c in CASES} == {16, 5, 24, 80}
    assert {c[1] for c in CASES} | fams >= set(HM.VARIANTS)
    for f in ("records_d8", "generic", "d5_scalar"):                       # every kind at every width in the three families
        assert {(c[2], c[4]) for c in CASES if c[0] == f and c[1] == "plain" and c[3] == HM.SOFTMAX and c[5] == "relu"} >= \
            {(k, w) for k in HM.KINDS for w in HM.WIDTHS}
    assert {c[2] for c in CASES if c[5] == "lrelu"} == set(HM.KINDS)
    assert any(c[3] == HM.BCE and c[4] == 80 for c in CASES) and any(c[3] == HM.MSE and c[4] == 16 for c in CASES)
    for v in HM.VARIANTS:                                                  # each variant once on a pair head and once on a node head
        kinds = {c[2] for c in CASES if c[1] == v or c[0] == v}
        assert "node" in kinds and any(k.startswith("pair") for k in kinds), v
    W1, b1, Wo = HM.head_values(8, 16, 5)
    assert W1.shape == (16, 8) and b1.shape == (16,) and Wo.shape == (5, 16) and np.all(b1 != 0) and np.abs(b1).max() <= 0.5


# -- header and bindings
def test_header_declares_the_feature():
    txt = open(HEADER).read()
    assert re.search(r"#define GAT_ABI_VERSION 6\b", txt)
    assert re.search(r"enum \{ GAT_HEAD_ACT_LRELU = 1 \};", txt)
    assert re.search(r"GAT_PARAM_HEAD_W = 8, GAT_PARAM_HEAD_B = 9\b", txt)
    assert re.search(r"GAT_TAP_HEAD_HIDDEN = 20\b", txt)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", txt), s
    assert "int gat_set_head_hidden(gat_ctx* ctx, int32_t width, int32_t flags);" in txt
    assert "int gat_head_hidden_info(gat_ctx* ctx, int32_t* width, int32_t* flags);" in txt


def test_abi_py_declares_the_feature_and_the_library_exports_it(pkg):
    A = pkg.abi
    src = open(os.path.join(os.path.dirname(A.__file__), "abi.py")).read()
    lib = A.load_library()
    for s in NEW_SYMBOLS:
        assert f'"{s}"' in src and s in A.declared_symbols(), s
        assert getattr(lib, s) is not None, s            # exported by the built library
    for s in A.declared_symbols():                       # and every other declared symbol still is
        assert hasattr(lib, s), s
    assert (A.PARAM_HEAD_W, A.PARAM_HEAD_B, A.TAP_HEAD_HIDDEN, A.HEAD_ACT_LRELU) == (8, 9, 20, 1)
    assert A.PARAM_GROUPS_ALL == tuple(range(10)) and A.PARAM_GROUPS == tuple(range(8))
    assert [A.head_act(a) for a in ("relu", "lrelu", 1)] == [0, 1, 1]
    with pytest.raises(ValueError):
        A.head_act("tanh")
    for name in ("set_head_hidden", "head_hidden_info"):
        assert callable(getattr(A.GatContext, name))
    assert callable(A.op_head_hidden_forward) and callable(A.op_head_hidden_backward)
    # the ctypes table matches the header's argument lists
    assert len(lib.gat_set_head_hidden.argtypes) == 3 and len(lib.gat_head_hidden_info.argtypes) == 3
    assert len(lib.gat_op_head_hidden_forward.argtypes) == 6 and len(lib.gat_op_head_hidden_backward.argtypes) == 7


# -- the host program: refused before any GPU call
def run(args):
    e = dict(os.environ)
    e.pop("DATA_ROOT", None)
    return subprocess.run([BIN] + args, capture_output=True, text=True, env=e, timeout=600)


def test_train_edge_head_hidden_refusals_and_help(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    base = ["--heads", "8,8", "--outdims", "8,8", "--dataset", "tiny", "--data-root", str(tmp_path)]
    for args, msg in ((base + ["--head-hidden", "16", "--ranks", "2"],
                       "Error: --head-hidden needs --ranks 1: the hidden layer in front of the output head has no sharded form\n"),
                      (base + ["--head-hidden", "0"], "Error: --head-hidden must be an integer K >= 1 (the hidden layer's width)\n"),
                      (base + ["--head-hidden", "-3"], "Error: --head-hidden must be an integer K >= 1 (the hidden layer's width)\n"),
                      (base + ["--head-hidden", "16x"], "Error: --head-hidden must be an integer K >= 1 (the hidden layer's width)\n"),
                      (base + ["--head-hidden"], "Error: --head-hidden must be an integer K >= 1 (the hidden layer's width)\n"),
                      (base + ["--head-hidden", "16", "--head-act", "tanh"], "Error: --head-act must be relu or lrelu\n")):
        r = run(args)
        assert r.returncode == 1 and r.stderr.endswith(msg), (args, r.stderr)
        assert "[Memory Tracker]" not in r.stdout and "Configuration:" not in r.stdout      # nothing touched the GPU
    text = run(["--help"]).stdout
    assert "--head-hidden K [--head-act relu|lrelu]" in text and "W1 and b1 follow We" in text
    top = open(os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "host", "train_edge.cpp")).read().split("#include", 1)[0]
    assert "--head-hidden K [--head-act relu|lrelu]" in top              # the comment block at the top
