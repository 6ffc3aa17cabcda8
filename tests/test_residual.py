"""Residual connections and per-layer bias on the GPU (include/gatv2_abi.h "residual"): off is off, parity of every dispatcher
family against the fp64 model of tests/step_ref.py (linear, bias, both; plain and with all three regularisers), empty and
emptied rows, a three-layer model, the step paths against each other, flat_lrelu_index, the optimizer, shards, error codes.

The graph is make_graph of tests/feature_cases.py: F = 24, C = 5, one empty row (3) and a hub row (7) of 300
in-edges that is processed as segments — the smallest shapes that reach the split-row combine and the empty-row case."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dropedge_ref as E
import feature_cases as FC
import parity
import step_ref as SR
from feature_cases import FAMILIES, REG, compare, make_ctx, make_graph, parity_graph, pick_case, setters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")

MODES = FC.RES_MODES
GROUPS = FC.GROUPS[:5]
TAPS = ["hpre"]


def all_grads(pkg, ctx):
    return FC.grads(pkg, ctx, GROUPS)


def test_off_is_off(pkg, orc):
    A = pkg.abi
    g = make_graph(1)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)

    def ctx_of(touch):
        return make_ctx(pkg, g, [8, 8], [8, 8], P, residual=(False, False) if touch else None, collect_timing=True)      # no flags
    with ctx_of(False) as a, ctx_of(True) as b:
        assert b.param_count(A.PARAM_WRES) == 0 and b.param_count(A.PARAM_B) == 0
        assert a.n_params == b.n_params
        for c in (a, b):
            c.kernel_stats_reset()
        ra, rb = a.step(), b.step()
        assert ra == rb
        for x, y in zip(all_grads(pkg, a), all_grads(pkg, b)):
            assert np.array_equal(x, y)
        for l in range(2):
            assert np.array_equal(a.tap(A.TAP_HPRE, l), b.tap(A.TAP_HPRE, l))
        sa, sb = a.kernel_stats(), b.kernel_stats()
        assert {k: v[0] for k, v in sa.items()} == {k: v[0] for k, v in sb.items()}      # the same launches, class by class
        assert a.algorithmic_bytes() == b.algorithmic_bytes()


@pytest.mark.parametrize("reg", [None, REG], ids=["plain", "regularised"])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("name,heads,outdims,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_parity_against_fp64(pkg, orc, name, heads, outdims, kw, mode, reg):
    g = parity_graph()
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    bf16 = kw.get("dtype") == "bf16"
    P, inp, ref = pick_case(orc, cfg, g, mode, reg=reg, bf16_pl=bf16)
    ref["loss"].backward()
    with make_ctx(pkg, g, heads, outdims, P, **inp, **setters(mode), reg=reg, **kw) as ctx:
        loss, _ = ctx.step()
        compare(pkg, ctx, g, cfg, ref, loss, 1e-2 if bf16 else 1e-4, TAPS, GROUPS)


@pytest.mark.parametrize("kw", [{}, {"keep_taps": True}], ids=["records", "keep_taps"])
def test_empty_and_emptied_rows(pkg, orc, kw):
    """The empty row (3) and the rows DropEdge empties have h_pre = Wres x' + b of the fp64 model, not 0, and their G reaches
    grad_b: the device's grad_b is closer to the model's than the empty row's own contribution is large."""
    A = pkg.abi
    g = parity_graph()
    heads, outdims = [8, 8], [8, 8]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    mode = MODES[2]
    seed, pe = 1, 0.9
    keeps = [E.edge_keep(seed, 1, l, g["row_ptr"], g["col_idx"], pe) for l in range(2)]
    deg = np.diff(g["row_ptr"])
    emptied = [np.flatnonzero((deg > 0) & (np.diff(E.reduce_graph(g["row_ptr"], g["col_idx"], k)[0]) == 0)) for k in keeps]
    assert all(len(e) >= 1 for e in emptied)
    P, inp, ref = pick_case(orc, cfg, g, mode, keeps=keeps)
    Wres, b = inp["Wres"], inp["b"]
    ref["loss"].backward()
    wo, bo = SR.res_offsets(cfg)
    with make_ctx(pkg, g, heads, outdims, P, **inp, **setters(mode), **kw) as ctx:
        ctx.set_dropout(0.0, 0.0, seed=seed)
        ctx.set_dropedge(pe)
        loss, _ = ctx.step()
        compare(pkg, ctx, g, cfg, ref, loss, 1e-4, TAPS, GROUPS)
        x0 = g["x"].astype(np.float64)
        hp0 = ctx.tap(A.TAP_HPRE, 0).reshape(g["n"], -1)
        want0 = x0 @ Wres[:wo[1]].astype(np.float64).reshape(64, g["f"]).T + b[:bo[1]]
        for r in [3] + list(emptied[0]):
            assert np.abs(hp0[r] - want0[r]).max() <= 1e-4 * np.abs(want0).max(), r
            assert np.abs(hp0[r]).max() > 0
        gb = ctx.grads_get(A.PARAM_B)
        for l in range(2):
            G3 = ref["hpre"][l].grad[3].numpy().reshape(-1)              # what the empty row adds to grad_b of layer l
            assert np.abs(G3).max() > 0
            err = np.abs(gb[bo[l]:bo[l + 1]] - ref["b"].grad.numpy()[bo[l]:bo[l + 1]]).max()
            parity.record(f"grad_b[{l}] / the empty row's share", err / np.abs(G3).max(), 0.1)
            assert err < 0.1 * np.abs(G3).max()


@pytest.mark.parametrize("reg", [None, REG], ids=["plain", "regularised"])
def test_three_layers(pkg, orc, reg):
    """[8,8,8] x [8,8,8]: the input gradient of a hidden layer carries G Wres through two layers."""
    g = parity_graph()
    heads, outdims = [8, 8, 8], [8, 8, 8]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P, inp, ref = pick_case(orc, cfg, g, MODES[2], reg=reg)
    ref["loss"].backward()
    with make_ctx(pkg, g, heads, outdims, P, **inp, **setters(MODES[2]), reg=reg) as ctx:
        loss, _ = ctx.step()
        compare(pkg, ctx, g, cfg, ref, loss, 1e-4, TAPS, GROUPS)


@pytest.mark.parametrize("name,heads,outdims,kw", [f for f in FAMILIES if f[0] in ("records_d8", "msg_rows_d16", "generic")],
                         ids=["records_d8", "msg_rows_d16", "generic"])
def test_paths_agree(pkg, orc, name, heads, outdims, kw):
    """gat_step = gat_forward + gat_backward within 1e-5; the phase API = gat_backward bitwise; a gat_step_graph replay = the
    eager step bitwise; two runs bitwise equal.  The generic family's layer 0 scatters gPL with float atomics (gatv2_abi.h "Limits":
    the generic kernels, with or without this feature), so the one group that scatter feeds — grad_W — is order-dependent at fp32
    round-off there and is held to 1e-5 of its max-abs instead; the four other groups, the new ones among them, stay bitwise."""
    g = make_graph(2)
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    Wres, b = SR.xavier_wres(cfg, 3)

    def new():
        return make_ctx(pkg, g, heads, outdims, P, Wres=Wres, b=b, **setters(MODES[2]), **kw)

    def same(xs, ys):
        for i, (x, y) in enumerate(zip(xs, ys)):
            if i == 0 and name == "generic":
                assert np.abs(x - y).max() <= 1e-5 * np.abs(y).max()
            else:
                assert np.array_equal(x, y), i
        return True
    with new() as s1, new() as s2, new() as fb, new() as ph, new() as gr:
        l1, l2 = s1.step(), s2.step()
        g1, g2 = all_grads(pkg, s1), all_grads(pkg, s2)
        assert l1 == l2 and same(g1, g2)                                                # two runs
        lf = fb.forward(); fb.backward()
        gf = all_grads(pkg, fb)
        assert abs(lf[0] - l1[0]) <= 1e-5 * max(1.0, abs(l1[0])) and lf[1] == l1[1]
        for x, y in zip(g1, gf):
            assert np.abs(x - y).max() <= 1e-5 * np.abs(y).max()
        for l in range(cfg.L):                                                          # the phase API
            ph.layer_project(l); ph.layer_forward_edges(l)
        lp = ph.head_forward(); ph.head_backward()
        for l in range(cfg.L - 1, -1, -1):
            ph.layer_backward_edges(l); ph.layer_backward_dense(l)
        assert lp == lf and same(all_grads(pkg, ph), gf)
        gr.step_graph(True)
        for k in range(3):                                                              # eager warm-up, capture + launch, replay
            gr.zero_grad()
            lg = gr.step()
            assert lg == l1, k
            assert same(all_grads(pkg, gr), g1), k


def test_flat_lrelu_index(pkg, orc):
    g = parity_graph()
    heads, outdims = [8, 8], [8, 8]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P, inp, ref = pick_case(orc, cfg, g, MODES[2], flat_lrelu_index=True)
    ref["loss"].backward()
    with make_ctx(pkg, g, heads, outdims, P, **inp, **setters(MODES[2]), flat_lrelu_index=True) as ctx:
        loss, _ = ctx.step()
        compare(pkg, ctx, g, cfg, ref, loss, 1e-4, TAPS, GROUPS)


def test_optimizer_moves_the_new_groups(pkg):
    """One clip + Adam step and one SGD step on values written straight into a residual context, against fp64 numpy at the bars
    of tests/test_optimizer.py (sgd: 1 ulp of max(|p|, |lr g|); adam: t (1e-5 lr + 2^-23 max|p|); clip: norm 1e-5, direction 2^-23)."""
    A = pkg.abi
    F32 = np.float32
    rng = np.random.default_rng(21)
    groups = (A.PARAM_W, A.PARAM_A, A.PARAM_WO, A.PARAM_WRES, A.PARAM_B)
    thr = 5.0
    lr, b1, b2, eps = (float(F32(v)) for v in (0.01, 0.9, 0.999, 1e-8))
    with pkg.GatContext([8, 4], [8, 4], 37, 3) as ctx:
        ctx.set_residual(linear=True, bias=True)
        counts = [ctx.param_count(k) for k in groups]
        assert counts[3] == 64 * 37 + 16 * 64 and counts[4] == 64 + 16 and ctx.n_params == sum(counts)
        p0 = [rng.standard_normal(n).astype(F32) for n in counts]
        gr = [(rng.standard_normal(n) * s).astype(F32) for n, s in zip(counts, (0.01, 0.01, 0.01, 0.5, 0.01))]   # only Wres above thr
        norms = [np.linalg.norm(x.astype(np.float64)) for x in gr]
        assert norms[3] > 2 * thr and all(nn < thr / 2 for i, nn in enumerate(norms) if i != 3)
        for k, p, x in zip(groups, p0, gr):
            ctx.params_set(k, p); ctx.grads_set(k, x)
        ctx.clip(thr)
        clipped = [ctx.grads_get(k) for k in groups]
        for i in (0, 1, 2, 4):                                 # below the threshold: untouched, each group by its own norm
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
    with pkg.GatContext([8, 4], [8, 4], 37, 3) as plain, pkg.GatContext([8, 4], [8, 4], 37, 3) as res:
        res.set_residual(linear=True, bias=True)
        plain.params_init(9); res.params_init(9)
        for k in (A.PARAM_W, A.PARAM_A, A.PARAM_WO):
            assert np.array_equal(plain.params_get(k), res.params_get(k))
        Wr, b = res.params_get(A.PARAM_WRES), res.params_get(A.PARAM_B)
        assert (b == 0).all()
        lim0, lim1 = np.sqrt(6 / (37 + 64)), np.sqrt(6 / (64 + 16))
        w0, w1 = Wr[:64 * 37], Wr[64 * 37:]
        assert 0.9 * lim0 < np.abs(w0).max() <= lim0 * (1 + 1e-6) and 0.9 * lim1 < np.abs(w1).max() <= lim1 * (1 + 1e-6)
        assert abs(w0.mean()) < 0.05 * lim0 and len(np.unique(Wr)) > 0.99 * Wr.size


@pytest.mark.parametrize("replicate", [False, True], ids=["exchange", "replicated_input"])
@pytest.mark.parametrize("world", [2, 3])
def test_shards_on_the_host_transport(pkg, orc, world, replicate):
    """`world` processes sharing one GPU equal the single-GPU gradients at 1e-5 (all five groups; the all-reduce sums the new ones)."""
    import torch.multiprocessing as mp
    g = FC.shard_problem()
    inp = FC.shard_inputs(orc, g, norm=False)
    with make_ctx(pkg, g, [8, 8], [8, 8], inp[:3], Wres=inp[3], b=inp[4], **setters(MODES[2])) as one:
        loss1, correct1 = one.step()
        want = np.concatenate(all_grads(pkg, one))
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(FC.shard_worker, args=(world, d, f"/gatv2_res_{os.getpid()}_{world}_{int(replicate)}", replicate, False), nprocs=world, join=True)
        outs = [np.load(os.path.join(d, f"r{r}.npz")) for r in range(world)]
    for o in outs:
        assert abs(float(o["loss"]) - loss1) <= 1e-5 * max(1.0, abs(loss1)) and int(o["correct"]) == correct1
        assert o["grads"].shape == want.shape
        parity.record("grads", parity.rel_err(o["grads"], want), 1e-5)
        assert np.abs(o["grads"] - want).max() <= 1e-5 * np.abs(want).max()
        assert np.array_equal(o["grads"], outs[0]["grads"])


def test_train_edge_ranks_with_residual(pkg, tmp_path):
    """train_edge --ranks 2 --residual --bias ends at the parameters of --ranks 1 (through --dump-params, which carries the new
    groups behind the others), and the flags change the run."""
    ds = pkg.synth.make_dataset("cora", scale=0.15)
    pkg.synth.write_text_dataset(ds, str(tmp_path), "tiny")
    base = ["--dataset", "tiny", "--data-root", str(tmp_path), "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8",
            "--epochs", "3", "--optimizer", "sgd", "--lr", "0.001", "--seed", "5", "--residual", "--bias"]
    env = dict(os.environ)
    env.pop("DATA_ROOT", None)
    one = subprocess.run([BIN] + base + ["--dump-params", str(tmp_path / "p1.bin")], capture_output=True, text=True, env=env, timeout=600)
    assert one.returncode == 0, one.stderr
    two = subprocess.run([BIN] + base + ["--ranks", "2", "--transport", "host", "--dump-params", str(tmp_path / "p2.bin")],
                         capture_output=True, text=True, env=env, timeout=600)
    assert two.returncode == 0, two.stderr
    plain = subprocess.run([BIN] + base[:-2] + ["--dump-params", str(tmp_path / "p0.bin")], capture_output=True, text=True, env=env, timeout=600)
    assert plain.returncode == 0, plain.stderr
    p0, p1, p2 = (np.fromfile(tmp_path / f, dtype=np.float32) for f in ("p0.bin", "p1.bin", "p2.bin"))
    f, c = ds["f"], ds["c"]
    n_old = 64 * 2 * f + 64 * 2 * 64 + 128 + c * 8
    assert p0.size == n_old and p1.size == n_old + 64 * f + 64 * 64 + 128 and p2.size == p1.size
    assert np.abs(p1 - p2).max() < 1e-4 * max(1.0, np.abs(p1).max())
    assert np.abs(p1[n_old:]).max() > 0 and not np.array_equal(p1[:n_old], p0)
    import re
    pat = r"Avg Loss: ([0-9.]+), Accuracy: ([0-9.]+)%"
    a, b = re.findall(pat, one.stdout), re.findall(pat, two.stdout)
    assert len(a) == 3 and len(b) == 3
    for (la, aa), (lb, ab) in zip(a, b):
        assert abs(float(la) - float(lb)) < 1e-4 and abs(float(aa) - float(ab)) < 0.011
    # a file written with the flags loads back with them
    again = subprocess.run([BIN] + base + ["--epochs", "1", "--load-params", str(tmp_path / "p1.bin")], capture_output=True, text=True,
                           env=env, timeout=600)
    assert again.returncode == 0, again.stderr


def test_errors(pkg, orc):
    A = pkg.abi
    g = make_graph(7)
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        for flags in (4, 8, 7, -1):
            with pytest.raises(A.GatError) as ei:
                ctx.set_residual(flags=flags)
            assert ei.value.code == 10001                    # GAT_E_INVALID
        ctx.set_residual(linear=True)                        # allowed, and again with other flags while nothing sized the buffers
        ctx.set_residual(linear=True, bias=True)
        assert ctx.param_count(A.PARAM_WRES) == 64 * g["f"] + 64 * 64 and ctx.param_count(A.PARAM_B) == 128
        ctx.params_set(A.PARAM_B, np.ones(128, np.float32))
        with pytest.raises(A.GatError) as ei:
            ctx.set_residual(linear=True)
        assert ei.value.code == 10002                        # GAT_E_STATE: after gat_params_set
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.set_graph(g["row_ptr"], g["col_idx"])
        with pytest.raises(A.GatError) as ei:
            ctx.set_residual(bias=True)
        assert ei.value.code == 10002                        # after gat_set_graph
        with pytest.raises(A.GatError) as ei:
            ctx.set_residual()                               # flags == 0 too: the rule is about the call order
        assert ei.value.code == 10002
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.grads_get(A.PARAM_W)
        with pytest.raises(A.GatError) as ei:
            ctx.set_residual(bias=True)
        assert ei.value.code == 10002                        # after gat_grads_get
