"""Edge features without a GPU (include/gatv2_abi.h "edge features"): the edge term of the fp64 model of tests/step_ref.py: zero
weights against the model without them (and tests/torch_ref.py), gradWe against central finite differences, the new ABI constants and symbols, the shard
and synth helpers, and — a condition, not a skip — a parameter seed clear of the LeakyReLU kinks among the first 40 for every parity
case tests/test_edge_features.py runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import edge_feat_ref as EF
import feature_cases as FC
import step_ref as SR
import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")

# plain / all three regularisers / residual + norm
FORMS = [("plain", False, False), ("reg", True, False), ("res_norm", False, True)]


def _inputs(orc, g, cfg, reg, res_norm, ps=3):
    P = orc.xavier_params(cfg, ps)
    keeps, attn, feat = FC.masks(cfg, g, cfg.heads, FC.REG if reg else None)
    kw = dict(keeps=keeps, attn=attn, feat=feat, eps=FC.EPS)
    if res_norm:
        kw["Wres"], kw["b"] = SR.xavier_wres(cfg, ps)
        kw["gamma"], kw["beta"] = SR.ln_params(cfg, ps)
    return P, kw


@pytest.mark.parametrize("name,reg,res_norm", FORMS, ids=[f[0] for f in FORMS])
def test_zero_edge_weights_are_the_model_without_the_term(orc, name, reg, res_norm):
    """ea with We = 0 is the model without the arguments, value for value, and in its plain form that model is tests/torch_ref.py's.
    (With a non-zero We the model is held to the recorded forms edge_* of tests/test_step_ref_cpu.py.)"""
    g = FC.host_graph(1)
    cfg = orc.Config([4, 2], [4, 8], g["f"], g["c"])
    P, kw = _inputs(orc, g, cfg, reg, res_norm)
    want = FC.run_model(cfg, g, P, **kw)
    want["loss"].backward()
    fe = 3
    groups = [k for k in FC.GROUPS[:7] if want[k] is not None]
    assert len(groups) == (7 if res_norm else 3) and want["We"] is None
    got = FC.run_model(cfg, g, P, ea=EF.edge_attrs(g, fe), We=np.zeros(SR.we_offsets(cfg, fe)[-1], np.float32), **kw)
    assert got["loss"].item() == want["loss"].item()
    assert got["s_min"] == want["s_min"] and got["hpre_min"] == want["hpre_min"] and got["v_min"] == want["v_min"]
    got["loss"].backward()
    for k in groups:
        assert np.array_equal(got[k].grad.numpy(), want[k].grad.numpy()), k
    for l in range(cfg.L):
        assert np.array_equal(got["hpre"][l].detach().numpy(), want["hpre"][l].detach().numpy())
        assert np.array_equal(got["alpha"][l], want["alpha"][l])
    assert got["We"] is not None
    if name == "plain":
        ref = torch_ref.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P)
        ref["loss"].backward()
        assert abs(got["loss"].item() - ref["loss"].item()) <= 1e-12 * abs(ref["loss"].item())
        for x, y in zip(got["hpre"], ref["hpre"]):
            assert (x - y).abs().max().item() <= 1e-12
        for k in groups:
            assert (got[k].grad - ref[k].grad).abs().max().item() <= 1e-12 * max(1.0, ref[k].grad.abs().max().item())


def test_the_edge_term_is_in_the_score_only(orc):
    """score[l] = sum_d a * LReLU(PL[src] + PR[dst] + We ea) restated with numpy from the projections; a non-zero We changes the loss."""
    g = FC.host_graph(2)
    cfg = orc.Config([4, 2], [4, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 1)
    fe = 3
    ea, We = EF.edge_attrs(g, fe), SR.xavier_we(cfg, fe, 1)
    ref = SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, ea=ea, We=We)
    base = FC.run_model(cfg, g, P)
    assert abs(ref["loss"].item() - base["loss"].item()) > 1e-3
    W, a = P[0].astype(np.float64), P[1].astype(np.float64)
    H, D, F = cfg.heads[0], cfg.outdims[0], g["f"]
    Wl = W[cfg.w_offsets[0]:cfg.w_offsets[1]].reshape(H * D, 2 * F)
    x = g["x"].astype(np.float64)
    dst = np.repeat(np.arange(g["n"]), np.diff(g["row_ptr"]))
    s = x[g["col_idx"]] @ Wl[:, :F].T + x[dst] @ Wl[:, F:].T + ea.astype(np.float64) @ We[:H * D * fe].astype(np.float64).reshape(H * D, fe).T
    sc = (a[:H * D] * np.where(s > 0, s, 0.01 * s)).reshape(-1, H, D).sum(-1).T
    assert ref["score"][0].shape == (H, len(dst)) and np.abs(ref["score"][0] - sc).max() <= 1e-12
    assert g["row_ptr"][3] == g["row_ptr"][4] and ref["hpre"][0][3].abs().max().item() == 0       # a row without in-edges is unaffected


def test_grad_we_matches_central_differences(orc):
    g = FC.host_graph(4, n=25, e=120)
    cfg = orc.Config([2, 2], [3, 4], g["f"], g["c"])
    P = orc.xavier_params(cfg, 2)
    fe = 3
    ea = EF.edge_attrs(g, fe)
    We = SR.xavier_we(cfg, fe, 2).astype(np.float64)
    keeps, attn, feat = FC.masks(cfg, g, cfg.heads, FC.REG)

    def run(w):
        return SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, ea=ea, We=w, keeps=keeps, attn=attn, feat=feat)
    ref = run(We)
    assert ref["s_min"] > 1e-4 and ref["hpre_min"] > 1e-4      # the probes below stay on one side of every kink
    ref["loss"].backward()
    grad = ref["We"].grad.numpy()
    assert grad.shape == We.shape and np.abs(grad).max() > 0
    o = SR.we_offsets(cfg, fe)
    assert all(np.abs(grad[o[l]:o[l + 1]]).max() > 0 for l in range(cfg.L))
    rng = np.random.default_rng(0)
    h = 1e-6
    for i in rng.choice(We.size, 16, replace=False):
        up, dn = We.copy(), We.copy()
        up[i] += h; dn[i] -= h
        fd = (run(up)["loss"].item() - run(dn)["loss"].item()) / (2 * h)
        assert abs(fd - grad[i]) <= 1e-6 * max(1.0, np.abs(grad).max()), (i, fd, grad[i])


def test_dropped_edges_get_no_gradient(orc):
    """gradWe of a DropEdge step is gradWe of the model on the reduced graph with the reduced attribute rows (same mask in both layers)."""
    import dropedge_ref as E
    g = FC.host_graph(3)
    cfg = orc.Config([4, 2], [4, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 1)
    fe = 2
    ea, We = EF.edge_attrs(g, fe), SR.xavier_we(cfg, fe, 1)
    keep = np.random.default_rng(5).random(len(g["col_idx"])) > 0.5
    full = SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, ea=ea, We=We, keeps=[keep, keep])
    rp, ci = E.reduce_graph(g["row_ptr"], g["col_idx"], keep)
    red = SR.forward(cfg, rp, ci, g["labels"], g["x"], *P, ea=ea[keep], We=We)
    full["loss"].backward(); red["loss"].backward()
    assert np.abs(full["We"].grad.numpy() - red["We"].grad.numpy()).max() <= 1e-12 * np.abs(red["We"].grad.numpy()).max()


def test_constants_and_symbols(pkg):
    A = pkg.abi
    assert A.PARAM_WE == 7 and A.PARAM_GROUPS == tuple(range(8))
    lib = ctypes.CDLL(A.LIB_PATH)
    for name in ("gat_set_edge_dim", "gat_set_edge_features", "gat_set_edge_features_device"):
        assert name in A.declared_symbols() and hasattr(lib, name), name
    assert A.load_library().gat_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "gatv2_abi.h")).read()
    assert "#define GAT_ABI_VERSION 6" in hdr
    assert "GAT_PARAM_LN_G = 5, GAT_PARAM_LN_B = 6, GAT_PARAM_WE = 7 };" in hdr
    assert "int gat_set_edge_dim(gat_ctx* ctx, int32_t edge_dim);" in hdr
    assert f"#define GAT_EDGE_DIM_MAX {A.EDGE_DIM_MAX}" in hdr
    for m in ("set_edge_dim", "set_edge_features", "set_edge_features_device"):
        assert hasattr(pkg.GatContext, m)


def test_shard_helper_slices_the_local_csr_order(pkg):
    S = pkg.shard
    g = FC.shard_problem()
    E = len(g["col_idx"])
    ea = np.arange(E * 2, dtype=np.float32).reshape(E, 2)
    seen = []
    for world in (2, 3):
        parts = []
        for rank in range(world):
            plan = S.make_plan(g["row_ptr"], world, rank)
            rp, ci = S.local_csr(plan, g["row_ptr"], g["col_idx"])
            loc = S.local_edge_features(plan, g["row_ptr"], ea)
            assert loc.shape == (len(ci), 2) and loc.flags["C_CONTIGUOUS"]
            # local edge k of local row r is global edge row_ptr[row0 + r] + (k - rp[r])
            e0 = int(g["row_ptr"][plan.row0])
            assert np.array_equal(loc[:, 0], ea[e0:e0 + len(ci), 0])
            assert np.array_equal(plan.from_table_ids(ci), g["col_idx"][e0:e0 + len(ci)])
            parts.append(loc)
        assert np.array_equal(np.concatenate(parts), ea)
        seen.append(world)
    with pytest.raises(ValueError):
        S.local_edge_features(S.make_plan(g["row_ptr"], 2, 0), g["row_ptr"], ea[:-1])
    assert seen == [2, 3]


def test_synth_edge_features_are_deterministic(pkg):
    f = pkg.synth.edge_features
    a, b = f(7, 1000, 5), f(7, 1000, 5)
    assert a.shape == (1000, 5) and a.dtype == np.float32 and np.array_equal(a, b)
    assert not np.array_equal(a, f(8, 1000, 5)) and abs(float(a.mean())) < 0.1 and 0.9 < float(a.std()) < 1.1
    assert f(7, 0, 3).shape == (0, 3)
    with pytest.raises(ValueError):
        f(7, 10, 0)


# -- the seed condition: every case of lists 1 and 2 of tests/test_edge_features.py finds its parameters among the first 40 seeds
@pytest.mark.parametrize("name,heads,outdims,kw", FC.FAMILIES, ids=[f[0] for f in FC.FAMILIES])
def test_families_find_a_clear_seed(orc, name, heads, outdims, kw):
    g = FC.parity_graph()
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    for fe in EF.FES:
        for reg in (None, FC.REG):
            EF.pick(FC, orc, cfg, g, fe, reg, bf16=kw.get("dtype") == "bf16")


@pytest.mark.parametrize("dt", FC.DTYPES)
@pytest.mark.parametrize("hd,d", FC.SHAPES, ids=[f"hd{hd}_d{d}" for hd, d in FC.SHAPES])
def test_shapes_find_a_clear_seed(orc, hd, d, dt):
    g, heads, outdims, cfg = FC.shape_model(orc, hd, d)
    _, inp, ref = EF.pick(FC, orc, cfg, g, EF.SHAPE_FE, FC.REG, res_norm=True, bf16=dt == "bf16")
    ref["loss"].backward()
    assert np.abs(ref["We"].grad.numpy()).max() > 1e-3          # not vacuous


def test_rows_case_finds_a_clear_seed(orc):
    """The two models of test_dropedge_rows_and_dropped_edges: per-layer masks at p_e = 0.9, and one mask on the reduced graph."""
    import dropedge_ref as E
    g = FC.parity_graph()
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    fe = 3
    _, inp, ref = EF.pick(FC, orc, cfg, g, fe, None, keeps=FC.rows_keeps(g))
    keep = E.edge_keep(FC.ROWS_SEED, 1, 0, g["row_ptr"], g["col_idx"], FC.ROWS_PE, shared=True)
    assert 0 < keep.sum() < keep.size
    rp, ci = E.reduce_graph(g["row_ptr"], g["col_idx"], keep)
    assert (np.diff(rp)[np.diff(g["row_ptr"]) > 0] == 0).any()          # rows go empty
    FC.pick_params(orc, cfg, lambda ps, PP: (None, SR.forward(cfg, rp, ci, g["labels"], g["x"], *PP, ea=inp["ea"][keep],
                                                              We=SR.xavier_we(cfg, fe, ps))), FC.CLEAR_HPRE)


def test_train_edge_flag_and_its_refusals(tmp_path):
    out = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--edge-features" in out.stdout
    base = [BIN, "--dataset", "none", "--data-root", str(tmp_path), "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8", "--edge-features"]
    for extra, word in ((["--add-self-loops"], "rebuild the graph"), (["--undirected"], "rebuild the graph"), (["--coalesce"], "rebuild the graph"),
                        (["--ranks", "2", "--transport", "host"], "--ranks 1")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--edge-features" in r.stderr and word in r.stderr, (extra, r.stderr)


def test_write_text_dataset_writes_the_attribute_rows(pkg, tmp_path):
    ds = pkg.synth.make_dataset("cora", scale=0.05)
    ds["edge_features"] = pkg.synth.edge_features(3, len(ds["col_idx"]), 4)
    d = pkg.synth.write_text_dataset(ds, str(tmp_path), "tiny")
    back = np.loadtxt(os.path.join(d, "edge_features.txt"), dtype=np.float32, ndmin=2)
    assert back.shape == ds["edge_features"].shape and np.array_equal(back, ds["edge_features"])
    assert not os.path.exists(os.path.join(pkg.synth.write_text_dataset(dict(ds, edge_features=None), str(tmp_path), "plain"), "edge_features.txt"))
