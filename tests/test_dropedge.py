"""DropEdge on the GPU (include/gatv2_abi.h "DropEdge"): off is off, the mask tap against the numpy hash, parity of every
dispatcher family against the fp64 model on the reduced graph, equivalence with a plain step on the reduced graph, emptied rows,
eval mode / counter / resume / graph replay, error paths, shards, the full Products shape."""
import os
import re
import subprocess

import numpy as np
import pytest

import dropedge_ref as E
import dropout_ref as R
import feature_cases as FC
from feature_cases import FAMILIES, make_ctx, make_graph

pytestmark = pytest.mark.gpu
WAWO = ["W", "a", "Wo"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")


def test_off_is_off(pkg, orc):
    g = make_graph(1)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    with make_ctx(pkg, g, [8, 8], [8, 8], P) as a, make_ctx(pkg, g, [8, 8], [8, 8], P) as b:
        b.set_dropedge(0.0, keep_self=True, shared_layers=True)
        ra, rb = a.step(), b.step()
        assert ra == rb
        for x, y in zip(FC.grads(pkg, a, WAWO), FC.grads(pkg, b, WAWO)):
            assert np.array_equal(x, y)
        assert b.dropout_step() == 0                         # nothing runs, nothing advances


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("keep_self", [False, True])
def test_mask_tap_equals_the_numpy_hash(pkg, orc, keep_self, shared):
    A = pkg.abi
    g = make_graph(2, self_loops=True)
    heads, outdims = [8, 4], [8, 16]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    seed = 0x1234_5678_9ABC
    with make_ctx(pkg, g, heads, outdims, orc.xavier_params(cfg, 1)) as ctx:
        ctx.set_dropout(0.0, 0.0, seed=seed, first_step=0)   # seeds only
        ctx.set_dropedge(0.4, keep_self=keep_self, shared_layers=shared)
        hub = slice(int(g["row_ptr"][7]), int(g["row_ptr"][8]))
        assert hub.stop - hub.start == 300                   # longer than a segment: positions span the segments
        taps = []
        for step in (1, 2):
            ctx.step()
            assert ctx.dropout_step() == step
            for l in range(2):
                want = E.edge_keep(seed, step, l, g["row_ptr"], g["col_idx"], 0.4, keep_self=keep_self, shared=shared)
                got = ctx.tap(A.TAP_EDGE_KEEP, l)
                assert got.shape == (len(g["col_idx"]),)
                assert np.array_equal(got, want.astype(np.float32)), (step, l)
                assert 0 < got[hub].sum() < 300
                taps.append(got)
        assert np.array_equal(taps[0], taps[1]) == shared    # layers 0 and 1 of step 1
        assert not np.array_equal(taps[0], taps[2])          # steps 1 and 2
        if keep_self:
            ne = np.diff(g["row_ptr"]) > 0
            assert (taps[0][g["row_ptr"][:-1][ne]] == 1).all()


def test_without_set_dropout_seed_and_counter_are_zero(pkg, orc):
    A = pkg.abi
    g = make_graph(2)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    with make_ctx(pkg, g, [8, 8], [8, 8], orc.xavier_params(cfg, 1)) as ctx:
        ctx.set_dropedge(0.3)
        assert ctx.dropout_step() == 0
        ctx.step()
        assert ctx.dropout_step() == 1
        want = E.edge_keep(0, 1, 1, g["row_ptr"], g["col_idx"], 0.3)
        assert np.array_equal(ctx.tap(A.TAP_EDGE_KEEP, 1), want.astype(np.float32))


@pytest.mark.parametrize("pa,pf", [(0.0, 0.0), (0.3, 0.5)])
@pytest.mark.parametrize("name,heads,outdims,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_parity_against_fp64(pkg, orc, name, heads, outdims, kw, pa, pf):
    """One mask per step for all layers, so that the model is dropedge_ref.forward: the step model on ONE reduced graph."""
    pe, seed = 0.4, 77
    g = make_graph(5, n=150, e=700)              # small enough that some Xavier seed keeps every |s|, |h_pre| off the kink
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    keep = E.edge_keep(seed, 1, 0, g["row_ptr"], g["col_idx"], pe, shared=True)
    hub = slice(int(g["row_ptr"][7]), int(g["row_ptr"][8]))
    assert 0 < keep[hub].sum() < 300 and not keep[hub][256:].all()      # the hub's segments both lose edges
    attn = [R.attn_factor(seed, 1, l, g["row_ptr"], heads[l], pa) for l in range(cfg.L)] if pa > 0 else None
    feat = [R.feat_factor(seed, 1, l, g["n"], cfg.in_dims[l], pf) for l in range(cfg.L)] if pf > 0 else None
    bf16 = kw.get("dtype") == "bf16"
    P, ref = FC.pick_params(orc, cfg, lambda ps, P: (E.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, keep=keep,
                                                               attn=attn, feat=feat, bf16_pl=bf16),), FC.CLEAR_HPRE)
    ref["loss"].backward()
    tol = 1e-2 if bf16 else 1e-4
    with make_ctx(pkg, g, heads, outdims, P, **kw) as ctx:
        ctx.set_dropout(pf, pa, seed=seed, first_step=0)
        ctx.set_dropedge(pe, shared_layers=True)
        loss, _ = ctx.step()
        assert ctx.dropout_step() == 1           # once per forward, whichever regularisers are on
        FC.compare(pkg, ctx, g, cfg, ref, loss, tol, taps=["hpre"], groups=WAWO)
        if kw.get("keep_taps"):                  # alpha: exactly 0 at dropped edges, rows of survivors sum to 1
            A = pkg.abi
            for tap in (A.TAP_ALPHA, A.TAP_GE, A.TAP_GALPHA):
                assert (ctx.tap(tap, 0)[:, ~keep] == 0).all()
            al = ctx.tap(A.TAP_ALPHA, 0)
            rp, _ = E.reduce_graph(g["row_ptr"], g["col_idx"], keep)
            sums = np.add.reduceat(al[:, keep], rp[:-1][np.diff(rp) > 0], axis=1)
            assert np.abs(sums - 1).max() < 1e-4


@pytest.mark.parametrize("name,heads,outdims,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_parity_with_a_mask_per_layer(pkg, orc, name, heads, outdims, kw):
    """Independent draws per layer (the default), together with attention and feature dropout, over every family."""
    pe, pa, pf, seed = 0.4, 0.3, 0.5, 78
    bf16 = kw.get("dtype") == "bf16"
    g = make_graph(5, n=150, e=700)
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    keeps = [E.edge_keep(seed, 1, l, g["row_ptr"], g["col_idx"], pe) for l in range(cfg.L)]
    assert not np.array_equal(keeps[0], keeps[1])
    attn = [R.attn_factor(seed, 1, l, g["row_ptr"], heads[l], pa) for l in range(cfg.L)]
    feat = [R.feat_factor(seed, 1, l, g["n"], cfg.in_dims[l], pf) for l in range(cfg.L)]
    P, ref = FC.pick_params(orc, cfg, lambda ps, P: (FC.run_model(cfg, g, P, keeps=keeps, attn=attn, feat=feat, bf16_pl=bf16),),
                            FC.CLEAR_HPRE)
    ref["loss"].backward()
    with make_ctx(pkg, g, heads, outdims, P, **kw) as ctx:
        ctx.set_dropout(pf, pa, seed=seed, first_step=0)
        ctx.set_dropedge(pe)
        loss, _ = ctx.step()
        FC.compare(pkg, ctx, g, cfg, ref, loss, 1e-2 if bf16 else 1e-4, taps=["hpre"], groups=WAWO)


@pytest.mark.parametrize("name,heads,outdims,kw", [f for f in FAMILIES if f[0] in ("records_d8", "msg_rows_d16", "generic", "keep_taps")],
                         ids=["records_d8", "msg_rows_d16", "generic", "keep_taps"])
def test_equivalence_with_the_reduced_graph(pkg, orc, name, heads, outdims, kw):
    """A DropEdge step computes what a plain step computes on the CSR with the dropped edges removed (not bitwise: chunk
    boundaries move)."""
    A = pkg.abi
    pe, seed = 0.4, 31
    g = make_graph(8)
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    keep = E.edge_keep(seed, 1, 0, g["row_ptr"], g["col_idx"], pe, shared=True)
    rp, ci = E.reduce_graph(g["row_ptr"], g["col_idx"], keep)
    g2 = dict(g, row_ptr=rp, col_idx=ci)
    with make_ctx(pkg, g, heads, outdims, P, **kw) as a, make_ctx(pkg, g2, heads, outdims, P, **kw) as b:
        a.set_dropout(0.0, 0.0, seed=seed)
        a.set_dropedge(pe, shared_layers=True)
        (la, ca), (lb, cb) = a.step(), b.step()
        print("loss", la, lb)
        assert abs(la - lb) / g["n"] < 1e-4 and ca == cb
        for l in range(cfg.L):
            x, y = a.tap(A.TAP_HPRE, l), b.tap(A.TAP_HPRE, l)
            print("hpre", l, np.abs(x - y).max(), np.abs(y).max())
            assert np.abs(x - y).max() <= 1e-4 * np.abs(y).max()
        for x, y in zip(FC.grads(pkg, a, WAWO), FC.grads(pkg, b, WAWO)):
            print("grad", np.abs(x - y).max(), np.abs(y).max())
            assert np.abs(x - y).max() <= 1e-4 * np.abs(y).max()
        if kw.get("keep_taps"):
            for l in range(cfg.L):
                al = a.tap(A.TAP_ALPHA, l)
                assert (al[:, ~keep] == 0).all()
                assert np.abs(al[:, keep] - b.tap(A.TAP_ALPHA, l)).max() < 1e-4
                for tap in (A.TAP_GE, A.TAP_GALPHA):
                    t = a.tap(tap, l)
                    assert (t[:, ~keep] == 0).all()
                    want = b.tap(tap, l)
                    assert np.abs(t[:, keep] - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-30)


@pytest.mark.parametrize("kw", [{}, {"keep_taps": True}], ids=["records", "keep_taps"])
def test_row_that_loses_all_its_edges(pkg, orc, kw):
    A = pkg.abi
    g = make_graph(9)
    heads, outdims = [8, 8], [8, 8]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    seed = 1
    deg = np.diff(g["row_ptr"])
    keeps = [E.edge_keep(seed, 1, l, g["row_ptr"], g["col_idx"], 0.9) for l in range(2)]
    emptied = []
    for k in keeps:
        left = np.diff(E.reduce_graph(g["row_ptr"], g["col_idx"], k)[0])
        emptied.append(np.flatnonzero((deg > 0) & (left == 0)))
        assert len(emptied[-1]) >= 1             # from the numpy mask: this seed empties non-empty rows
    with make_ctx(pkg, g, heads, outdims, orc.xavier_params(cfg, 2), **kw) as ctx:
        ctx.set_dropout(0.0, 0.0, seed=seed)
        ctx.set_dropedge(0.9)
        loss, _ = ctx.step()
        assert np.isfinite(loss)
        for l in range(2):
            hp = ctx.tap(A.TAP_HPRE, l)
            assert np.isfinite(hp).all()
            assert (hp[emptied[l]] == 0).all()
            assert (hp[3] == 0).all()            # the row that was empty to begin with
            if kw.get("keep_taps"):              # the statistics of a zero in-degree row (row 3 is one)
                mx, sm = ctx.tap(A.TAP_MAX, l), ctx.tap(A.TAP_SUM, l)
                assert (mx[:, emptied[l]] == mx[:, [3]]).all() and (sm[:, emptied[l]] == 0).all()
                assert (ctx.tap(A.TAP_ALPHA, l)[:, ~keeps[l]] == 0).all()
        for x in FC.grads(pkg, ctx, WAWO):
            assert np.isfinite(x).all() and np.abs(x).max() > 0


def test_eval_mode_and_counter(pkg, orc):
    A = pkg.abi
    g = make_graph(3)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 2)
    with make_ctx(pkg, g, [8, 8], [8, 8], P) as plain, make_ctx(pkg, g, [8, 8], [8, 8], P) as ctx:
        ctx.set_dropedge(0.5)
        ctx.set_training(False)
        assert ctx.forward() == plain.forward()
        for l in range(2):
            assert np.array_equal(ctx.tap(A.TAP_HPRE, l), plain.tap(A.TAP_HPRE, l))
        assert ctx.dropout_step() == 0
        ctx.set_training(True)
        assert ctx.forward() != plain.forward()
        assert ctx.dropout_step() == 1
        ctx.step()
        assert ctx.dropout_step() == 2
        ctx.set_dropout(0.5, 0.5, seed=0, first_step=2)      # all three on: still one advance per forward
        ctx.step()
        assert ctx.dropout_step() == 3
        ctx.step_graph(True)
        for k in range(3):                       # eager warm-up, capture + launch, replay
            ctx.step()
            assert ctx.dropout_step() == 4 + k
        ctx.step_graph(False)
        for l in range(2):                       # the phase API
            ctx.layer_project(l); ctx.layer_forward_edges(l)
        ctx.head_forward(want_loss=False); ctx.head_backward()
        for l in (1, 0):
            ctx.layer_backward_edges(l); ctx.layer_backward_dense(l)
        assert ctx.dropout_step() == 7


def test_first_step_resumes_the_sequence(pkg, orc):
    g = make_graph(4)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 2)

    def run(first, k):
        out = []
        with make_ctx(pkg, g, [8, 8], [8, 8], P) as ctx:
            ctx.set_dropedge(0.5, keep_self=True)            # before set_dropout: the order does not matter
            ctx.set_dropout(0.0, 0.0, seed=9, first_step=first)
            for _ in range(k):
                ctx.zero_grad()
                out.append((ctx.step(), FC.grads(pkg, ctx, WAWO)))
        return out
    a, b = run(0, 7), run(5, 2)
    for (la, ga), (lb, gb) in zip(a[5:], b):
        assert la == lb and all(np.array_equal(x, y) for x, y in zip(ga, gb))
    assert a[0][0] != a[1][0]                    # consecutive steps draw different masks


def test_graph_replay_equals_eager(pkg, orc):
    g = make_graph(6)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 4)
    with make_ctx(pkg, g, [8, 8], [8, 8], P) as e, make_ctx(pkg, g, [8, 8], [8, 8], P) as r:
        for c in (e, r):
            c.set_dropout(0.0, 0.0, seed=21, first_step=0)
            c.set_dropedge(0.5)
        r.step_graph(True)
        losses = []
        for _ in range(3):
            e.zero_grad(); r.zero_grad()
            le, lr = e.step(), r.step()
            assert le == lr
            losses.append(le)
            for x, y in zip(FC.grads(pkg, e, WAWO), FC.grads(pkg, r, WAWO)):
                assert np.array_equal(x, y)
        assert len(set(losses)) == 3             # a replay draws fresh masks


def test_errors(pkg, orc):
    A = pkg.abi
    g = make_graph(7)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    with make_ctx(pkg, g, [8, 8], [8, 8], orc.xavier_params(cfg, 1)) as ctx:
        for p, flags in ((1.0, 0), (-0.1, 0), (float("nan"), 0), (0.5, 8), (0.0, 8), (0.5, 4)):
            with pytest.raises(A.GatError) as ei:
                ctx.set_dropedge(p, flags=flags)
            assert ei.value.code == 10001                    # GAT_E_INVALID
        ctx.set_dropedge(0.5, flags=3)                       # both known bits
    with pkg.GatContext([8, 8], [8, 8], 16, 4) as ctx:       # allowed before the graph is set
        ctx.set_dropedge(0.25, keep_self=True)


@pytest.mark.parametrize("ranks", [2, 3])
def test_train_edge_ranks_with_dropedge(pkg, tmp_path, ranks):
    """train_edge --ranks P --transport host: destination-range shards own whole rows and key the draws by the unsharded node
    id, so the epochs print the single-GPU numbers and end at the same parameters (self-loops: table_row0 + row on a shard)."""
    ds = pkg.synth.make_dataset("cora", scale=0.15)
    pkg.synth.write_text_dataset(ds, str(tmp_path), "tiny")
    base = ["--dataset", "tiny", "--data-root", str(tmp_path), "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8",
            "--epochs", "3", "--optimizer", "sgd", "--lr", "0.001", "--seed", "5", "--add-self-loops",
            "--drop-edge", "0.5", "--drop-edge-keep-self"]
    env = dict(os.environ)
    env.pop("DATA_ROOT", None)
    one = subprocess.run([BIN] + base + ["--dump-params", str(tmp_path / "p1.bin")], capture_output=True, text=True, env=env, timeout=600)
    assert one.returncode == 0, one.stderr
    many = subprocess.run([BIN] + base + ["--ranks", str(ranks), "--transport", "host", "--dump-params", str(tmp_path / "pN.bin")],
                          capture_output=True, text=True, env=env, timeout=600)
    assert many.returncode == 0, many.stderr
    pat = r"Avg Loss: ([0-9.]+), Accuracy: ([0-9.]+)%"
    a = [(float(m.group(1)), float(m.group(2))) for m in re.finditer(pat, one.stdout)]
    b = [(float(m.group(1)), float(m.group(2))) for m in re.finditer(pat, many.stdout)]
    assert len(a) == 3 and len(b) == 3
    for (la, aa), (lb, ab) in zip(a, b):
        assert abs(la - lb) < 1e-4 and abs(aa - ab) < 0.011
    p1 = np.fromfile(tmp_path / "p1.bin", dtype=np.float32)
    pN = np.fromfile(tmp_path / "pN.bin", dtype=np.float32)
    assert np.abs(p1 - pN).max() < 1e-4 * max(1.0, np.abs(p1).max())
    # without the flags the run differs: the mask does something; and keep-self differs from plain DropEdge
    plain = subprocess.run([BIN] + base[:-3], capture_output=True, text=True, env=env, timeout=600)
    assert plain.returncode == 0 and re.findall(pat, plain.stdout) != re.findall(pat, one.stdout)
    noself = subprocess.run([BIN] + base[:-1], capture_output=True, text=True, env=env, timeout=600)
    assert noself.returncode == 0 and re.findall(pat, noself.stdout) != re.findall(pat, one.stdout)


def test_products_full_size(pkg):
    import torch
    A = pkg.abi
    dev = torch.device("cuda", 0)
    dsd = pkg.synth.make_dataset_device("products", dev)
    rp = dsd["row_ptr"]
    d_rp = torch.from_numpy(np.ascontiguousarray(rp, np.int32)).to(dev)
    n, e = dsd["n"], dsd["e"]
    ctx = pkg.GatContext([8, 8], [8, 8], dsd["f"], dsd["c"])
    try:
        ctx.set_graph_device(d_rp.data_ptr(), dsd["d_col_idx"].data_ptr(), n, e)
        ctx.set_features_device(dsd["d_x"].data_ptr(), n, dsd["f"])
        ctx.set_labels_device(dsd["d_labels"].data_ptr(), n)
        ctx.params_init(42)
        ctx.set_dropedge(0.5)                    # a mask per layer
        outs = []
        for _ in range(2):                       # the same step twice: bitwise equal
            ctx.set_dropout(0.0, 0.0, seed=3, first_step=0)
            ctx.zero_grad()
            outs.append((ctx.step(), FC.grads(pkg, ctx, WAWO)))
        assert outs[0][0] == outs[1][0]
        assert all(np.array_equal(x, y) for x, y in zip(outs[0][1], outs[1][1]))
        assert all(np.isfinite(x).all() for x in outs[0][1])
        keep = ctx.tap(A.TAP_EDGE_KEEP, 1) != 0  # [E] of the last layer
        rate = float(keep.mean())
        print("keep rate", rate, keep.size)
        assert abs(rate - 0.5) < 5 * np.sqrt(0.25 / keep.size), rate
        # h_pre of 1,000 rows (the largest hub among them) against fp64 from the PL / PR taps, dropped edges removed
        PL, PR = ctx.tap(A.TAP_PL, 1).astype(np.float64), ctx.tap(A.TAP_PR, 1).astype(np.float64)
        hpre = ctx.tap(A.TAP_HPRE, 1)
        a1 = ctx.params_get(A.PARAM_A)[64:128].astype(np.float64).reshape(8, 8)
        col = dsd["d_col_idx"].cpu().numpy()
        deg = np.diff(rp)
        rng = np.random.default_rng(0)
        rows = np.unique(np.concatenate([[int(deg.argmax())], rng.integers(0, n, 999)]))
        err = scale = 0.0
        for r in rows:
            b0, b1 = int(rp[r]), int(rp[r + 1])
            src = col[b0:b1][keep[b0:b1]]
            want = np.zeros((8, 8))
            if len(src) > 0:
                s = PL[src].reshape(-1, 8, 8) + PR[r].reshape(8, 8)
                sc = (a1 * np.maximum(s, 0.01 * s)).sum(-1)                     # [deg, H]
                pe = np.exp(sc - np.maximum(sc.max(0), -1e9))
                alpha = pe / (pe.sum(0) + 1e-8)
                want = np.einsum("eh,ehk->hk", alpha, PL[src].reshape(-1, 8, 8))
            err = max(err, float(np.abs(hpre[r] - want).max()))
            scale = max(scale, float(np.abs(want).max()))
        print("hpre err", err, "scale", scale)
        assert scale > 0 and err <= 1e-4 * scale, (err, scale)
    finally:
        ctx.close()
