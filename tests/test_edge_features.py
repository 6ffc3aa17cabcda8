"""Edge features in the attention score on the GPU (include/gatv2_abi.h "edge features"): parity of every dispatcher family and every
fast-path shape against the fp64 model of tests/step_ref.py, DropEdge rows, off is off, We = 0, the step paths against each other,
the optimizer, shards, error codes.

Each parity case is one context and one step on parity_graph of tests/feature_cases.py (150 nodes, 700 edges + a hub row of 300
in-edges that is processed as segments, one empty row) at the project's bars: 1e-4 of max-abs for fp32, 1e-2 for bf16 storage.
tests/test_edge_features_cpu.py proves on the host that every case of the two matrices has a parameter seed clear of the LeakyReLU
kinks among the first 40."""
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dropedge_ref as E
import edge_feat_ref as EF
import feature_cases as FC
import parity
import step_ref as SR
from feature_cases import FAMILIES, REG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")

TOL = {"fp32": 1e-4, "bf16": 1e-2}
compare_all = EF.compare_all                      # with check_we: shared with tests/pick_profiles.py

# -- 1. families
@pytest.mark.parametrize("reg", [None, REG], ids=["plain", "regularised"])
@pytest.mark.parametrize("fe", EF.FES, ids=[f"fe{f}" for f in EF.FES])
@pytest.mark.parametrize("name,heads,outdims,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_families_against_fp64(pkg, orc, name, heads, outdims, kw, fe, reg):
    A = pkg.abi
    g = FC.parity_graph()
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    bf16 = kw.get("dtype") == "bf16"
    tol = TOL["bf16" if bf16 else "fp32"]
    P, inp, ref = EF.pick(FC, orc, cfg, g, fe, reg, bf16=bf16)
    ref["loss"].backward()
    with EF.make_ctx(pkg, g, heads, outdims, P, fe, **inp, reg=reg, **kw) as ctx:
        assert ctx.param_count(A.PARAM_WE) == SR.we_offsets(cfg, fe)[-1]
        loss, _ = ctx.step()
        compare_all(pkg, ctx, g, cfg, ref, loss, tol)
        if kw.get("keep_taps"):
            for l in range(cfg.L):
                keep = ref["alpha"][l][0] != 0                       # the model's surviving edges
                assert keep.sum() > 0 and (reg is None) == bool(keep.all())
                if reg is not None:
                    assert np.array_equal(keep, ctx.tap(A.TAP_EDGE_KEEP, l) != 0)
                parity.check_rel(f"alpha[{l}]", ctx.tap(A.TAP_ALPHA, l), ref["alpha"][l], tol)
                parity.check_rel(f"score[{l}]", ctx.tap(A.TAP_SCORE, l)[:, keep], ref["score"][l][:, keep], tol)      # with the edge term


# -- 2. shapes
SHAPE_CASES = list(itertools.product(FC.SHAPES, FC.DTYPES))


@pytest.mark.parametrize("shape,dt", SHAPE_CASES, ids=[f"hd{s[0]}_d{s[1]}-{dt}" for s, dt in SHAPE_CASES])
def test_shapes_against_fp64(pkg, orc, shape, dt):
    """Every (H*D, D) of the wave-per-row kernels x both storage modes at Fe = 5, norm + both residual flags + all three regularisers."""
    hd, d = shape
    g, heads, outdims, cfg = FC.shape_model(orc, hd, d)
    P, inp, ref = EF.pick(FC, orc, cfg, g, EF.SHAPE_FE, REG, res_norm=True, bf16=dt == "bf16")
    ref["loss"].backward()
    kw = {"dtype": "bf16"} if dt == "bf16" else {}
    with EF.make_ctx(pkg, g, heads, outdims, P, EF.SHAPE_FE, **inp, reg=REG, **kw) as ctx:
        loss, _ = ctx.step()
        compare_all(pkg, ctx, g, cfg, ref, loss, TOL[dt])


# -- 3. rows
def test_dropedge_rows_and_dropped_edges(pkg, orc):
    """DropEdge at p_e = 0.9 (rows go empty): everything still matches the model with the per-layer masks; and with ONE mask for both
    layers gradWe equals the model's on the REDUCED graph with the reduced attribute rows — a dropped edge's gPE is zero."""
    A = pkg.abi
    g = FC.parity_graph()
    heads, outdims, fe = [8, 8], [8, 8], 3
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    keeps = FC.rows_keeps(g)
    P, inp, ref = EF.pick(FC, orc, cfg, g, fe, None, keeps=keeps)
    ref["loss"].backward()
    with EF.make_ctx(pkg, g, heads, outdims, P, fe, **inp) as ctx:
        ctx.set_dropout(0.0, 0.0, seed=FC.ROWS_SEED)
        ctx.set_dropedge(FC.ROWS_PE)
        loss, _ = ctx.step()
        for l in range(2):
            assert np.array_equal(ctx.tap(A.TAP_EDGE_KEEP, l) != 0, keeps[l])
        compare_all(pkg, ctx, g, cfg, ref, loss, 1e-4)
    keep = E.edge_keep(FC.ROWS_SEED, 1, 0, g["row_ptr"], g["col_idx"], FC.ROWS_PE, shared=True)
    assert 0 < keep.sum() < keep.size
    rp, ci = E.reduce_graph(g["row_ptr"], g["col_idx"], keep)
    gr = dict(g, row_ptr=rp, col_idx=ci)
    ea = inp["ea"]
    P, inp, ref = FC.pick_params(orc, cfg, lambda ps, PP: (
        dict(We=SR.xavier_we(cfg, fe, ps)),
        SR.forward(cfg, rp, ci, g["labels"], g["x"], *PP, ea=ea[keep], We=SR.xavier_we(cfg, fe, ps))), FC.CLEAR_HPRE)
    ref["loss"].backward()
    with EF.make_ctx(pkg, g, heads, outdims, P, fe, ea=ea, **inp) as ctx:      # the FULL graph and the FULL attribute rows
        ctx.set_dropout(0.0, 0.0, seed=FC.ROWS_SEED)
        ctx.set_dropedge(FC.ROWS_PE, shared_layers=True)
        loss, _ = ctx.step()
        compare_all(pkg, ctx, gr, cfg, ref, loss, 1e-4)


# -- 4. off is off
def test_off_is_off(pkg, orc):
    A = pkg.abi
    g = FC.make_graph(1)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)

    def ctx_of(touch):
        return EF.make_ctx(pkg, g, [8, 8], [8, 8], P, 0, touch=touch, collect_timing=True)        # set_edge_dim(0), or no call at all
    with ctx_of(False) as a, ctx_of(True) as b:
        assert b.param_count(A.PARAM_WE) == 0 and a.n_params == b.n_params
        b.set_edge_features(np.zeros((len(g["col_idx"]), 0), np.float32))      # 0 floats per edge on both sides: nothing happens
        for c in (a, b):
            c.kernel_stats_reset()
        ra, rb = a.step(), b.step()
        assert ra == rb
        for k in A.PARAM_GROUPS:
            assert np.array_equal(a.grads_get(k), b.grads_get(k))
        for l in range(2):
            assert np.array_equal(a.tap(A.TAP_HPRE, l), b.tap(A.TAP_HPRE, l))
        sa, sb = a.kernel_stats(), b.kernel_stats()
        assert {k: v[0] for k, v in sa.items()} == {k: v[0] for k, v in sb.items()}      # the same launches, class by class
        assert a.algorithmic_bytes() == b.algorithmic_bytes()
    # on: the byte model adds exactly the four documented terms per layer
    fe = 4
    with EF.make_ctx(pkg, g, [8, 8], [8, 8], P, 0) as a, EF.make_ctx(pkg, g, [8, 8], [8, 8], P, fe) as b:
        (ta, pa), (tb, pb) = a.algorithmic_bytes(), b.algorithmic_bytes()
        Ecount, HD, L = len(g["col_idx"]), 64, 2
        add = {"project_gemm": Ecount * fe + HD * fe + Ecount * HD, "edge_forward": Ecount * HD, "edge_backward": 2 * Ecount * HD,
               "grad_w_gemm": Ecount * HD + Ecount * fe + HD * fe}
        for k in pa:
            assert pb[k] - pa[k] == 4.0 * L * add.get(k, 0), k
        assert tb - ta == 4.0 * L * sum(add.values())


# -- 5. We = 0
@pytest.mark.parametrize("kw", [{}, {"keep_taps": True}], ids=["records", "keep_taps"])
def test_zero_we_is_the_context_without_the_feature(pkg, orc, kw):
    """PE is an exact zero added to the score: loss and h_pre bitwise those of a context without the feature."""
    A = pkg.abi
    g = FC.parity_graph()
    heads, outdims, fe = [8, 8], [8, 8], 3
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    with EF.make_ctx(pkg, g, heads, outdims, P, 0, touch=False, **kw) as a, \
            EF.make_ctx(pkg, g, heads, outdims, P, fe, ea=EF.edge_attrs(g, fe), We=np.zeros(SR.we_offsets(cfg, fe)[-1], np.float32), **kw) as b:
        ra, rb = a.step(), b.step()
        assert ra == rb
        for l in range(2):
            assert np.array_equal(a.tap(A.TAP_HPRE, l), b.tap(A.TAP_HPRE, l))
        assert np.abs(b.grads_get(A.PARAM_WE)).max() > 0             # the gradient with respect to We is not zero at We = 0


# -- 6. paths agree
def test_paths_agree(pkg, orc):
    """gat_step, gat_forward + gat_backward, the phase API and a gat_step_graph replay give the same bits on a records family; a second
    step after zero_grad reproduces the first step's gradWe (the shared gPE buffer is rewritten, not accumulated)."""
    A = pkg.abi
    g = FC.make_graph(2)
    heads, outdims, fe = [8, 8], [8, 8], 3
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    ea, We = EF.edge_attrs(g, fe), SR.xavier_we(cfg, fe, 3)

    def new():
        return EF.make_ctx(pkg, g, heads, outdims, P, fe, ea=ea, We=We)

    def grads(c):
        return [c.grads_get(k) for k in A.PARAM_GROUPS]

    def same(xs, ys):
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert np.array_equal(x, y), i
        return True
    with new() as s1, new() as fb, new() as ph, new() as gr:
        l1 = s1.step()
        g1 = grads(s1)
        assert np.abs(g1[A.PARAM_WE]).max() > 0
        lf = fb.forward(); fb.backward()
        gf = grads(fb)
        for name, x, y in zip(FC.GROUPS[:8], g1, gf):
            if y.size:
                parity.record(f"step vs forward+backward: {name}", parity.rel_err(x, y), 0.0)
        assert lf == l1 and same(g1, gf)
        for l in range(cfg.L):                                                          # the phase API
            ph.layer_project(l); ph.layer_forward_edges(l)
        lp = ph.head_forward(); ph.head_backward()
        for l in range(cfg.L - 1, -1, -1):
            ph.layer_backward_edges(l); ph.layer_backward_dense(l)
        assert lp == lf and same(grads(ph), gf)
        gr.step_graph(True)
        for k in range(3):                                                              # eager warm-up, capture + launch, replay
            gr.zero_grad()
            lg = gr.step()
            assert lg == l1, k
            assert same(grads(gr), g1), k
        s1.zero_grad()                                                                  # two consecutive steps reuse gPE
        assert s1.step() == l1 and same(grads(s1), g1)


# -- 7. optimizer
def test_optimizer_moves_we(pkg):
    """One clip + Adam step and one SGD step on values written straight into an edge-feature context, against fp64 numpy at the bars
    of tests/test_optimizer.py (sgd: 1 ulp of max(|p|, |lr g|); adam: t (1e-5 lr + 2^-23 max|p|); clip: norm 1e-5, direction 2^-23)."""
    A = pkg.abi
    F32 = np.float32
    rng = np.random.default_rng(22)
    groups = (A.PARAM_W, A.PARAM_A, A.PARAM_WO, A.PARAM_WE)
    thr = 5.0
    lr, b1, b2, eps = (float(F32(v)) for v in (0.01, 0.9, 0.999, 1e-8))
    fe = 7
    with pkg.GatContext([8, 4], [8, 4], 37, 3) as ctx:
        ctx.set_edge_dim(fe)
        counts = [ctx.param_count(k) for k in groups]
        assert counts[3] == 64 * fe + 16 * fe and ctx.n_params == sum(counts)
        p0 = [rng.standard_normal(n).astype(F32) for n in counts]
        gr = [(rng.standard_normal(n) * s).astype(F32) for n, s in zip(counts, (0.01, 0.01, 0.01, 2.0))]         # only We above thr
        norms = [np.linalg.norm(x.astype(np.float64)) for x in gr]
        assert norms[3] > 2 * thr and all(nn < thr / 2 for nn in norms[:3])
        for k, p, x in zip(groups, p0, gr):
            ctx.params_set(k, p); ctx.grads_set(k, x)
        ctx.clip(thr)
        clipped = [ctx.grads_get(k) for k in groups]
        for i in range(3):                                     # below the threshold: untouched, each group by its own norm
            assert np.array_equal(clipped[i].view(np.uint32), gr[i].view(np.uint32))
        c64, w64 = clipped[3].astype(np.float64), gr[3].astype(np.float64)
        assert abs(np.linalg.norm(c64) / thr - 1.0) <= 1e-5
        s = float(c64 @ w64) / float(w64 @ w64)
        assert 0 < s < 1 and float((np.abs(c64 - s * w64) / np.maximum(np.abs(c64), 1e-30)).max()) <= 2.0 ** -23
        ctx.step_adam(lr, b1, b2, eps, 1)
        pmax = max(float(np.abs(p).max()) for p in p0) + 3.2 * lr
        after = []
        for k, p, x in zip(groups, p0, clipped):
            want = p.astype(np.float64)
            FC.adam64(want, x.astype(np.float64), np.zeros(len(p)), np.zeros(len(p)), lr, b1, b2, eps, 1)
            got = ctx.params_get(k)
            assert float(np.abs(got - want).max()) <= 1e-5 * lr + 2.0 ** -23 * pmax, k
            assert float(np.abs(got - p).max()) > 0.5 * lr        # the group moved
            after.append(got)
        slr = F32(0.37)
        ctx.step_sgd(float(slr))
        for k, p, x in zip(groups, after, clipped):
            step = np.float64(slr) * x.astype(np.float64)
            want = p.astype(np.float64) - step
            ulp = np.spacing(np.maximum(np.abs(p), np.abs(step).astype(F32))).astype(np.float64)
            assert float((np.abs(ctx.params_get(k) - want) / ulp).max()) <= 1.0, k
        ctx.zero_grad()
        assert all((ctx.grads_get(k) == 0).all() for k in groups)


def test_params_init_keeps_the_other_groups(pkg):
    A = pkg.abi
    fe = 5
    with pkg.GatContext([8, 4], [8, 4], 37, 3) as plain, pkg.GatContext([8, 4], [8, 4], 37, 3) as res:
        plain.set_residual(linear=True, bias=True)
        res.set_residual(linear=True, bias=True); res.set_edge_dim(fe)
        plain.params_init(9); res.params_init(9)
        for k in (A.PARAM_W, A.PARAM_A, A.PARAM_WO, A.PARAM_WRES, A.PARAM_B):
            assert np.array_equal(plain.params_get(k), res.params_get(k))
        assert plain.param_count(A.PARAM_WE) == 0
        We = res.params_get(A.PARAM_WE)
        lim0, lim1 = np.sqrt(6 / (fe + 64)), np.sqrt(6 / (fe + 16))
        w0, w1 = We[:64 * fe], We[64 * fe:]
        assert w1.size == 16 * fe
        assert 0.9 * lim0 < np.abs(w0).max() <= lim0 * (1 + 1e-6) and 0.85 * lim1 < np.abs(w1).max() <= lim1 * (1 + 1e-6)
        assert abs(w0.mean()) < 0.1 * lim0 and len(np.unique(We)) > 0.99 * We.size


# -- 8. shards
@pytest.mark.parametrize("world", [2, 3])
def test_shards_on_the_host_transport(pkg, orc, world):
    """`world` processes sharing one GPU equal the single-GPU loss and gradients at 1e-5 (all groups; the all-reduce sums the new one),
    the attribute rows cut by shard.local_edge_features."""
    import torch.multiprocessing as mp
    A = pkg.abi
    g = FC.shard_problem()
    inp, ea, We = EF.shard_inputs(orc, g)
    with EF.make_ctx(pkg, g, [8, 8], [8, 8], inp[:3], EF.SHARD_FE, ea=ea, We=We, Wres=inp[3], b=inp[4]) as one:
        loss1, correct1 = one.step()
        want = np.concatenate([one.grads_get(k) for k in A.PARAM_GROUPS])
        assert np.abs(one.grads_get(A.PARAM_WE)).max() > 0
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(EF.shard_worker, args=(world, d, f"/gatv2_ef_{os.getpid()}_{world}"), nprocs=world, join=True)
        outs = [np.load(os.path.join(d, f"r{r}.npz")) for r in range(world)]
    for o in outs:
        assert abs(float(o["loss"]) - loss1) <= 1e-5 * max(1.0, abs(loss1)) and int(o["correct"]) == correct1
        assert o["grads"].shape == want.shape
        parity.record("grads", parity.rel_err(o["grads"], want), 1e-5)
        assert np.abs(o["grads"] - want).max() <= 1e-5 * np.abs(want).max()
        assert np.array_equal(o["grads"], outs[0]["grads"])


# -- 9. errors
def test_errors(pkg, orc):
    A = pkg.abi
    INVALID, STATE = 10001, 10002
    g = FC.make_graph(7)
    Ecount = len(g["col_idx"])

    def raises(code, fn, *args, **kw):
        with pytest.raises(A.GatError) as ei:
            fn(*args, **kw)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        return str(ei.value)
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        for bad in (-1, A.EDGE_DIM_MAX + 1, 1 << 20):
            raises(INVALID, ctx.set_edge_dim, bad)
        ctx.set_edge_dim(A.EDGE_DIM_MAX)                     # the cap itself, and again while nothing sized the buffers
        ctx.set_edge_dim(3)
        ctx.set_residual(bias=True); ctx.set_norm()          # any order with the other two
        assert ctx.param_count(A.PARAM_WE) == 2 * 64 * 3
        raises(STATE, ctx.set_edge_features, np.zeros((Ecount, 3), np.float32))        # before the graph
        ctx.params_set(A.PARAM_B, np.ones(128, np.float32))
        raises(STATE, ctx.set_edge_dim, 4)                   # after gat_params_set
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.set_graph(g["row_ptr"], g["col_idx"])
        raises(STATE, ctx.set_edge_dim, 3)                   # after gat_set_graph
        raises(STATE, ctx.set_edge_dim, 0)                   # 0 too: the rule is about the call order
        raises(INVALID, ctx.set_edge_features, np.zeros((Ecount, 3), np.float32))      # the context has edge_dim 0
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.grads_get(A.PARAM_W)
        raises(STATE, ctx.set_edge_dim, 3)                   # after gat_grads_get
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.set_edge_dim(3)
        ctx.set_graph(g["row_ptr"], g["col_idx"]); ctx.set_features(g["x"]); ctx.set_labels(g["labels"])
        ctx.params_init(1)
        raises(INVALID, ctx.set_edge_features, np.zeros((Ecount, 4), np.float32))      # another edge_dim
        raises(INVALID, ctx.set_edge_features, np.zeros((Ecount - 1, 3), np.float32))  # another edge count
        raises(INVALID, ctx.set_edge_features_device, 0, Ecount, 3)                    # null pointer
        for call in (ctx.step, ctx.forward, lambda: ctx.layer_project(0), lambda: ctx.layer_forward_edges(0),
                     lambda: ctx.layer_backward_edges(1), lambda: ctx.layer_backward_dense(1)):
            assert "edge features not set" in raises(STATE, call)                      # and the text says so
        ctx.set_edge_features(np.zeros((Ecount, 3), np.float32))
        ctx.set_edge_features(EF.edge_attrs(g, 3))                                     # replaced by a later call
        loss, _ = ctx.step()
        assert np.isfinite(loss) and np.abs(ctx.grads_get(A.PARAM_WE)).max() > 0


SNIPPET = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as entry
import edge_feat_ref as EF, feature_cases as FC, step_ref as SR
pkg = entry.load_package(); orc = entry.load_oracle(); A = pkg.abi
g = FC.make_graph(2)
cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
P = orc.xavier_params(cfg, 3)
try:
    with EF.make_ctx(pkg, g, [8, 8], [8, 8], P, 3, ea=EF.edge_attrs(g, 3), We=SR.xavier_we(cfg, 3, 3)) as ctx:
        loss = ctx.forward()
        ctx.backward()
        np.save({out!r}, np.concatenate([ctx.grads_get(k) for k in A.PARAM_GROUPS]))
        print("LOSS", repr(loss[0]))
except A.GatError as e:
    print("CODE", e.code, "|", str(e)[:120])
"""


def test_choice_switches(pkg, orc, tmp_path):
    """The switches are read once per process, so each setting is a process of its own: GAT_BWD_ATOMICS=1 (no store path) is refused at
    the backward with GAT_E_UNSUPPORTED, as with dropout; the experiment library with GAT_DBG set refuses gat_set_edge_dim with the same
    code; GAT_PULL_LAST=1 (the last layer's decision-byte pull form, forced) does not
    apply to an edge-feature context — its gradients are bitwise those of the default settings."""
    from conftest import run_snippets_parallel
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jobs = {}
    exp = os.path.join(root, "graph-attention-network-gatv2-_amd", "libgatv2_hip_exp.so")
    assert os.path.exists(exp)
    for key, env in (("default", {}), ("atomics", {"GAT_BWD_ATOMICS": "1"}), ("pull_last", {"GAT_PULL_LAST": "1"}),
                     ("experiment", {"GATV2_LIB": exp, "GAT_DBG": "1"})):
        jobs[key] = (SNIPPET.format(root=root, tests=os.path.join(root, "tests"), out=str(tmp_path / f"{key}.npy")), env)
    res = run_snippets_parallel(jobs, workers=4, timeout=300)
    for key, r in res.items():
        assert r.returncode == 0, (key, r.stderr[-2000:])
    assert "CODE 10004" in res["atomics"].stdout and "edge_backward" in res["atomics"].stdout        # GAT_E_UNSUPPORTED, at the backward
    assert "CODE 10004" in res["experiment"].stdout and "gat_set_edge_dim" in res["experiment"].stdout  # the experiment library with GAT_DBG set
    assert "LOSS" in res["default"].stdout and res["default"].stdout == res["pull_last"].stdout
    a, b = np.load(tmp_path / "default.npy"), np.load(tmp_path / "pull_last.npy")
    assert np.abs(a).max() > 0 and np.array_equal(a, b)


def test_train_edge_with_edge_features(pkg, tmp_path):
    """train_edge --edge-features reads edge_features.txt, trains We (behind the other groups in --dump-params), reloads its own file,
    changes the run, and refuses an edges.txt dataset and a file of the wrong length with a text naming the reason."""
    fe = 3
    ds = pkg.synth.make_dataset("cora", scale=0.15)
    ds["edge_features"] = pkg.synth.edge_features(5, len(ds["col_idx"]), fe)
    pkg.synth.write_text_dataset(ds, str(tmp_path), "tiny")
    base = ["--dataset", "tiny", "--data-root", str(tmp_path), "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8",
            "--epochs", "3", "--optimizer", "sgd", "--lr", "0.01", "--seed", "5"]
    env = dict(os.environ)
    env.pop("DATA_ROOT", None)

    def run(args):
        return subprocess.run([BIN] + args, capture_output=True, text=True, env=env, timeout=600)
    plain = run(base + ["--dump-params", str(tmp_path / "p0.bin")])
    assert plain.returncode == 0, plain.stderr
    on = run(base + ["--edge-features", "--dump-params", str(tmp_path / "p1.bin")])
    assert on.returncode == 0, on.stderr
    assert f"Edge features: {fe} per edge" in on.stdout
    p0, p1 = (np.fromfile(tmp_path / f, dtype=np.float32) for f in ("p0.bin", "p1.bin"))
    f, c = ds["f"], ds["c"]
    n_old = 64 * 2 * f + 64 * 2 * 64 + 128 + c * 8
    assert p0.size == n_old and p1.size == n_old + 2 * 64 * fe
    We = p1[n_old:]
    lim = np.sqrt(6 / (fe + 64))
    assert np.abs(We).max() > 0.5 * lim and not np.array_equal(p1[:n_old], p0)      # the edge term changed the run
    # We moved from its initial value: one epoch at lr 0 dumps the initial parameters
    init = run(base[:-6] + ["--epochs", "1", "--optimizer", "sgd", "--lr", "0", "--seed", "5", "--edge-features", "--dump-params", str(tmp_path / "pi.bin")])
    assert init.returncode == 0, init.stderr
    pi = np.fromfile(tmp_path / "pi.bin", dtype=np.float32)
    assert pi.size == p1.size and np.abs(pi[n_old:]).max() <= lim * (1 + 1e-6) and np.abs(pi[n_old:] - We).max() > 0
    again = run(base + ["--epochs", "1", "--edge-features", "--load-params", str(tmp_path / "p1.bin")])
    assert again.returncode == 0, again.stderr
    # refusals
    np.savetxt(tmp_path / "tiny" / "edge_features.txt", ds["edge_features"][:-1], fmt="%.9g")
    short = run(base + ["--edge-features"])
    assert short.returncode != 0 and "edge_features.txt" in short.stderr
    dst = np.repeat(np.arange(ds["n"]), np.diff(ds["row_ptr"]))
    os.makedirs(tmp_path / "el")
    for name in ("features.txt", "labels.txt"):
        os.link(tmp_path / "tiny" / name, tmp_path / "el" / name)
    np.savetxt(tmp_path / "el" / "edges.txt", np.stack([ds["col_idx"], dst], 1), fmt="%d")
    np.savetxt(tmp_path / "el" / "edge_features.txt", ds["edge_features"], fmt="%.9g")
    el = run(["--dataset", "el"] + base[2:] + ["--edge-features"])
    assert el.returncode != 0 and "CSR dataset" in el.stderr
