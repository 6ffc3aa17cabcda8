"""Batch normalisation on the GPU (include/gatv2_abi.h "batch normalisation"): off is off; parity of every dispatcher family against
the fp64 model of tests/step_ref.py (BN only and BN + both residual flags; plain and with all three regularisers), loss, the
h_pre / hout / G taps of every layer, all seven gradient groups and the four statistics vectors; skip_last, three layers, rows wider
than a block's lanes; eval mode on the running statistics; the step paths against each other bit for bit, running statistics included;
one case per head kind; the optimizer; train_edge --batch-norm with its dump / load round trip; every refusal.

The graph is parity_graph of tests/feature_cases.py: 150 nodes, 700 edges, F = 24, C = 5, one empty row (3) and a hub row (7) of 300
in-edges that is processed as segments.  Tolerances are the project's bars: 1e-4 of max-abs, 1e-2 with bf16 storage."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import batchnorm_ref as BR
import bn_cases as BC
import feature_cases as FC
import parity
import step_ref as SR
from bn_cases import EPS, GROUPS, MODES, MOMENTUM, TAPS, make_ctx, pick_case, setters
from feature_cases import FAMILIES, REG, WIDE, make_graph, parity_graph, wide_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
INVALID, STATE, UNSUPPORTED = 10001, 10002, 10004


def all_grads(pkg, ctx):
    return FC.grads(pkg, ctx, GROUPS)


def test_off_is_off(pkg, orc):
    """gat_set_batch_norm(0, nan, nan) against an untouched context: loss and every gradient bitwise, the same launches class by class,
    the same algorithmic bytes, no norm groups, no statistics."""
    A = pkg.abi
    g = make_graph(1)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)

    def ctx_of(touch):                                       # flags == 0: eps and momentum are ignored
        return make_ctx(pkg, g, [8, 8], [8, 8], P, bn=dict(flags=0, eps=float("nan"), momentum=float("nan")) if touch else None, collect_timing=True)
    with ctx_of(False) as a, ctx_of(True) as b:
        assert b.param_count(A.PARAM_NORM_G) == 0 and b.param_count(A.PARAM_NORM_B) == 0
        assert b.batch_norm_info() == (0, 0.0, 0.0)
        assert a.n_params == b.n_params
        with pytest.raises(A.GatError) as ei:
            b.batch_norm_stats(A.BN_RUNNING_MEAN)
        assert ei.value.code == STATE
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
    tol = 1e-2 if bf16 else 1e-4
    P, inp, ref = pick_case(orc, cfg, g, mode, reg=reg, bf16_pl=bf16)
    ref["loss"].backward()
    with make_ctx(pkg, g, heads, outdims, P, **inp, **setters(mode), reg=reg, **kw) as ctx:
        loss, _ = ctx.step()
        BC.compare(pkg, ctx, g, cfg, ref, loss, tol)
        BC.compare_stats(pkg, ctx, ref, tol)


def test_skip_last(pkg, orc):
    """GAT_BN_SKIP_LAST: the last layer is the residual layer of always; its gamma / beta entries exist, are never read — NaN in them
    changes nothing — and their gradients are exactly 0; its statistics stay 0 / 1 / 0 / 0."""
    A = pkg.abi
    g = parity_graph()
    heads, outdims = [8, 8], [8, 8]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P, inp, ref = pick_case(orc, cfg, g, MODES[1], skip_last=True)
    ref["loss"].backward()
    gamma, beta = inp["gamma"].copy(), inp["beta"].copy()
    gamma[64:] = np.nan; beta[64:] = np.nan
    with make_ctx(pkg, g, heads, outdims, P, **dict(inp, gamma=gamma, beta=beta), **setters(MODES[1], skip_last=True)) as ctx:
        assert ctx.param_count(A.PARAM_NORM_G) == 128 and ctx.param_count(A.PARAM_NORM_B) == 128
        assert ctx.batch_norm_info()[0] == A.BN_ON | A.BN_SKIP_LAST
        loss, _ = ctx.step()
        BC.compare(pkg, ctx, g, cfg, ref, loss, 1e-4)
        BC.compare_stats(pkg, ctx, ref, 1e-4)
        for k in (A.PARAM_NORM_G, A.PARAM_NORM_B):
            assert (ctx.grads_get(k)[64:] == 0).all()
        for which, fresh in enumerate((0.0, 1.0, 0.0, 0.0)):
            assert (ctx.batch_norm_stats(which)[64:] == fresh).all()


@pytest.mark.parametrize("reg", [None, REG], ids=["plain", "regularised"])
def test_three_layers(pkg, orc, reg):
    g = parity_graph()
    heads, outdims = [8, 8, 8], [8, 8, 8]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P, inp, ref = pick_case(orc, cfg, g, MODES[1], reg=reg)
    ref["loss"].backward()
    with make_ctx(pkg, g, heads, outdims, P, **inp, **setters(MODES[1]), reg=reg) as ctx:
        loss, _ = ctx.step()
        BC.compare(pkg, ctx, g, cfg, ref, loss, 1e-4)
        BC.compare_stats(pkg, ctx, ref, 1e-4)


@pytest.mark.parametrize("name,heads,outdims", WIDE, ids=[w[0] for w in WIDE])
def test_wide_rows(pkg, orc, name, heads, outdims):
    g = wide_graph()
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P, inp, ref = pick_case(orc, cfg, g, MODES[1])
    ref["loss"].backward()
    with make_ctx(pkg, g, heads, outdims, P, **inp, **setters(MODES[1])) as ctx:
        loss, _ = ctx.step()
        BC.compare(pkg, ctx, g, cfg, ref, loss, 1e-4)
        BC.compare_stats(pkg, ctx, ref, 1e-4)


def _eval_case(orc, cfg, g, steps=3):
    """A seed whose eval pass on the running statistics after `steps` training steps is clear of the kinks (the training steps feed
    nothing but the statistics, which no kink moves).  -> P, inp, the eval model (before backward; "ran_on": the statistics it ran on)."""
    def after_steps(ps, P):
        Wres, b = SR.xavier_wres(cfg, ps)
        gamma, beta = SR.ln_params(cfg, ps)
        inp = dict(Wres=Wres, b=b, gamma=gamma, beta=beta)
        r = BC.run_model(cfg, g, P, **inp, eps=EPS, momentum=MOMENTUM)
        running = BR.stats_init(cfg)
        for _ in range(steps):                                # the parameters stand still: every step sees the same batch statistics
            running = BR.running_update(*running, r["batch_mean"], 1.0 / r["batch_rstd"] ** 2 - EPS, g["n"], MOMENTUM)
        ev = BC.run_model(cfg, g, P, **inp, eps=EPS, momentum=MOMENTUM, running=running, training=False)
        ev["ran_on"] = running
        return inp, ev
    return BC.pick_params(orc, cfg, after_steps, FC.CLEAR_V)


def test_eval_mode(pkg, orc):
    """After three training steps, set_training(False): the forward is the model's on the running statistics, gat_forward + gat_backward
    give the constant-statistics gradients, and nothing advances — the four vectors are bitwise what the training steps left.  Then
    stats_set followed by an eval forward uses the values set."""
    A = pkg.abi
    g = parity_graph()
    heads, outdims = [8, 8], [8, 8]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P, inp, ref = _eval_case(orc, cfg, g)
    ref["loss"].backward()
    with make_ctx(pkg, g, heads, outdims, P, **inp, **setters(MODES[1])) as ctx:
        for _ in range(3):
            ctx.zero_grad()
            ctx.step()
        parity.check_rel("running_mean after 3 steps", ctx.batch_norm_stats(A.BN_RUNNING_MEAN), ref["ran_on"][0], 1e-4)
        parity.check_rel("running_var after 3 steps", ctx.batch_norm_stats(A.BN_RUNNING_VAR), ref["ran_on"][1], 1e-4)
        before = BC.all_stats(ctx)
        ctx.set_training(False)
        ctx.zero_grad()
        loss, _ = ctx.forward()
        ctx.backward()
        BC.compare(pkg, ctx, g, cfg, ref, loss, 1e-4)
        for x, y in zip(before, BC.all_stats(ctx)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        # values of the caller's: the forward normalises with them
        rng = np.random.default_rng(8)
        mean, var = rng.uniform(-0.3, 0.3, 128).astype(np.float32), rng.uniform(0.5, 2.0, 128).astype(np.float32)
        ctx.set_batch_norm_stats(A.BN_RUNNING_MEAN, mean); ctx.set_batch_norm_stats(A.BN_RUNNING_VAR, var)
        assert np.array_equal(ctx.batch_norm_stats(A.BN_RUNNING_MEAN), mean) and np.array_equal(ctx.batch_norm_stats(A.BN_RUNNING_VAR), var)
        want = BC.run_model(cfg, g, P, **inp, eps=EPS, running=(mean, var), training=False)
        loss, _ = ctx.forward()
        assert abs(loss - want["loss"].item()) / g["n"] < 1e-4
        for l in range(2):
            w = want["hout"][l].detach().numpy()
            parity.check_rel(f"hout[{l}] on the statistics set", ctx.tap(A.TAP_HOUT, l).reshape(w.shape), w, 1e-4)
        assert np.array_equal(ctx.batch_norm_stats(A.BN_RUNNING_MEAN), mean)
        with pytest.raises(A.GatError) as ei:
            ctx.set_batch_norm_stats(A.BN_BATCH_MEAN, mean)
        assert ei.value.code == INVALID
        with pytest.raises(A.GatError) as ei:
            ctx.set_batch_norm_stats(A.BN_RUNNING_VAR, var[:64])
        assert ei.value.code == INVALID


def _bits(arrs):
    return [np.ascontiguousarray(a).view(np.uint32) for a in arrs]


@pytest.mark.parametrize("name,heads,outdims,kw", [f for f in FAMILIES if f[0] in ("records_d8", "msg_rows_d16", "generic")],
                         ids=["records_d8", "msg_rows_d16", "generic"])
def test_paths_agree(pkg, orc, name, heads, outdims, kw):
    """gat_step, a second run of it, gat_forward + gat_backward, the phase API and three replays of a captured step graph, three steps
    each: loss, every gradient group and the four statistics vectors bitwise after every step (generic: grad_W, fed by the edge
    backward's float-atomic scatter, at 1e-5 instead; the six other groups bitwise)."""
    g = make_graph(2)
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    Wres, b = SR.xavier_wres(cfg, 3)
    gamma, beta = SR.ln_params(cfg, 3)

    def new():
        return make_ctx(pkg, g, heads, outdims, P, Wres=Wres, b=b, gamma=gamma, beta=beta, **setters(MODES[1]), **kw)

    def same(xs, ys):
        for i, (x, y) in enumerate(zip(xs, ys)):
            if i == 0 and name == "generic":
                assert np.abs(x - y).max() <= 1e-5 * np.abs(y).max()
            else:
                assert np.array_equal(x, y), i
        return True

    def same_stats(x, y):
        return all(np.array_equal(p, q) for p, q in zip(_bits(BC.all_stats(x)), _bits(BC.all_stats(y))))
    with new() as s1, new() as s2, new() as fb, new() as ph, new() as gr:
        for k in range(3):                                   # the statistics advance: three steps on every path
            for c in (s1, s2, fb, ph, gr):
                c.zero_grad()
            if k == 0:
                gr.step_graph(True)                          # eager warm-up, capture + launch, replay
            l1, l2 = s1.step(), s2.step()
            g1, g2 = all_grads(pkg, s1), all_grads(pkg, s2)
            assert l1 == l2 and same(g1, g2) and same_stats(s1, s2)                     # two runs
            assert all(np.abs(x).max() > 0 for x in g1)
            lf = fb.forward(); fb.backward()
            gf = all_grads(pkg, fb)
            assert lf == l1 and same(g1, gf) and same_stats(s1, fb), k
            for l in range(cfg.L):                                                          # the phase API
                ph.layer_project(l); ph.layer_forward_edges(l)
            lp = ph.head_forward(); ph.head_backward()
            for l in range(cfg.L - 1, -1, -1):
                ph.layer_backward_edges(l); ph.layer_backward_dense(l)
            assert lp == lf and same(all_grads(pkg, ph), gf) and same_stats(ph, fb), k
            lg = gr.step()
            assert lg == l1 and same(all_grads(pkg, gr), g1) and same_stats(gr, s1), k
        mean = s1.batch_norm_stats(pkg.abi.BN_RUNNING_MEAN)
        first = BR.stats_init(cfg)[0]
        assert np.abs(mean).max() > 0 and not np.array_equal(mean, first)


RUN_TWICE = """
    import hashlib, sys
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import numpy as np
    import __graft_entry__ as entry
    import bn_cases as BC, feature_cases as FC, step_ref as SR
    pkg = entry.load_package(); orc = entry.load_oracle()
    g = FC.make_graph(2)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    Wres, b = SR.xavier_wres(cfg, 3); gamma, beta = SR.ln_params(cfg, 3)
    h = hashlib.sha256()
    with BC.make_ctx(pkg, g, [8, 8], [8, 8], P, Wres=Wres, b=b, gamma=gamma, beta=beta, reg=FC.REG, **BC.setters(BC.MODES[1])) as ctx:
        for k in range(2):
            ctx.zero_grad()
            loss = ctx.step()
            h.update(np.float32(loss[0]).tobytes())
            for a in FC.grads(pkg, ctx, FC.GROUPS[:7]) + BC.all_stats(ctx):
                h.update(np.ascontiguousarray(a).tobytes())
    print("DIGEST", h.hexdigest())
"""


def test_two_processes_agree_bitwise():
    code = textwrap.dedent(RUN_TWICE.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    outs = [subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300) for _ in range(2)]
    for o in outs:
        assert o.returncode == 0 and "DIGEST" in o.stdout, o.stderr[-2000:]
    assert outs[0].stdout.split("DIGEST")[1] == outs[1].stdout.split("DIGEST")[1]


@pytest.mark.parametrize("name", list(BC.HEAD_CASES))
def test_heads(pkg, orc, name):
    """One case per head kind on BN + both residual flags: loss over the rows that train, hout and G of every layer, the gradient
    groups (We, W1, b1 where the case has them), the statistics — which run over ALL rows under a training mask."""
    import head_mlp_ref as HM
    A = pkg.abi
    ci = BC.head_case(pkg, orc, name)
    ref = ci["ref"]
    ref["loss"].backward()
    with BC.make_head_ctx(pkg, ci) as ctx:
        loss, _ = ctx.step()
        BC.compare(pkg, ctx, dict(ci["g"], n=HM.loss_rows(ci)), ci["cfg"], ref, loss, 1e-4)
        BC.compare_stats(pkg, ctx, ref, 1e-4)
        for grp, key in ((A.PARAM_WE, "We"), (A.PARAM_HEAD_W, "W1"), (A.PARAM_HEAD_B, "b1")):
            got = ctx.grads_get(grp)
            if ref.get(key) is None:
                assert got.size == 0, key
            else:
                want = ref[key].grad.numpy().reshape(-1)
                assert got.shape == want.shape and np.abs(want).max() > 0, key
                parity.check_rel(f"grad {key}", got, want, 1e-4)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_optimizer_leaves_the_statistics_alone(pkg, orc, optimizer):
    """A training step, clip, an optimizer step, zero_grad: gamma and beta move, the four statistics vectors keep every bit."""
    A = pkg.abi
    g = parity_graph()
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    gamma, beta = SR.ln_params(cfg, 3)
    with make_ctx(pkg, g, [8, 8], [8, 8], P, gamma=gamma, beta=beta, **setters(MODES[0])) as ctx:
        ctx.step()
        stats = _bits(BC.all_stats(ctx))
        ctx.clip(5.0)
        grads = [ctx.grads_get(k) for k in (A.PARAM_NORM_G, A.PARAM_NORM_B)]
        assert all(np.abs(x).max() > 0 for x in grads)
        if optimizer == "sgd":
            ctx.step_sgd(0.05)
        else:
            ctx.step_adam(0.05, 0.9, 0.999, 1e-8, 1)
        ctx.zero_grad()
        assert not np.array_equal(ctx.params_get(A.PARAM_NORM_G), gamma) and not np.array_equal(ctx.params_get(A.PARAM_NORM_B), beta)
        for x, y in zip(stats, _bits(BC.all_stats(ctx))):
            assert np.array_equal(x, y)
        if optimizer == "sgd":
            want = gamma.astype(np.float64) - 0.05 * grads[0]
            assert np.abs(ctx.params_get(A.PARAM_NORM_G) - want).max() <= 1e-6


def test_params_init(pkg):
    A = pkg.abi
    with pkg.GatContext([8, 4], [8, 4], 37, 3) as plain, pkg.GatContext([8, 4], [8, 4], 37, 3) as bn:
        bn.set_batch_norm()
        plain.params_init(9); bn.params_init(9)
        for k in range(3):
            assert np.array_equal(plain.params_get(k), bn.params_get(k))
        assert (bn.params_get(A.PARAM_NORM_G) == 1).all() and bn.params_get(A.PARAM_NORM_G).size == 80
        assert (bn.params_get(A.PARAM_NORM_B) == 0).all() and bn.params_get(A.PARAM_NORM_B).size == 80
        assert (bn.batch_norm_stats(A.BN_RUNNING_MEAN) == 0).all() and (bn.batch_norm_stats(A.BN_RUNNING_VAR) == 1).all()
        flags, eps, mom = bn.batch_norm_info()
        assert flags == A.BN_ON and abs(eps - 1e-5) < 1e-12 and abs(mom - 0.1) < 1e-8


def test_train_edge_dump_load_round_trip(pkg, tmp_path):
    """train_edge --batch-norm: four epochs in one run equal two epochs, a dump, a load and two more — every printed training and
    validation line of epochs 3 and 4 character for character (the validation pass is an eval forward on the running statistics, so
    the file must carry them) and the final files bit for bit.  The file holds running_mean then running_var behind the last group,
    only with the flag; --batch-norm with --layer-norm is a usage error."""
    ds = pkg.synth.make_dataset("cora", scale=0.15)
    pkg.synth.write_text_dataset(ds, str(tmp_path), "tiny")
    n = ds["n"]
    val = np.random.default_rng(4).random(n) < 0.4
    np.savetxt(tmp_path / "val.txt", val.astype(int), fmt="%d")
    np.savetxt(tmp_path / "train.txt", (~val).astype(int), fmt="%d")
    base = ["--dataset", "tiny", "--data-root", str(tmp_path), "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8", "--optimizer", "sgd",
            "--lr", "0.05", "--seed", "5", "--train-mask", str(tmp_path / "train.txt"), "--val-mask", str(tmp_path / "val.txt"), "--batch-norm",
            "--bn-momentum", "0.3"]
    env = dict(os.environ)
    env.pop("DATA_ROOT", None)

    def run(args, ok=True):
        r = subprocess.run([BIN] + args, capture_output=True, text=True, env=env, timeout=600)
        assert (r.returncode == 0) == ok, r.stderr
        return r
    lines = lambda r: re.findall(r"^(?:Avg Loss|Val Loss).*$", r.stdout, flags=re.M)
    whole = run(base + ["--epochs", "4", "--dump-params", str(tmp_path / "p4.bin")])
    run(base + ["--epochs", "2", "--dump-params", str(tmp_path / "p2.bin")])
    rest = run(base + ["--epochs", "2", "--load-params", str(tmp_path / "p2.bin"), "--dump-params", str(tmp_path / "p22.bin")])
    a, b = lines(whole), lines(rest)
    assert len(a) == 8 and len(b) == 4 and any(ln.startswith("Val Loss") for ln in b)
    assert a[4:] == b, (a, b)
    p4, p2, p22 = (np.fromfile(tmp_path / f, dtype=np.float32) for f in ("p4.bin", "p2.bin", "p22.bin"))
    assert np.array_equal(p4.view(np.uint32), p22.view(np.uint32))
    f, c = ds["f"], ds["c"]
    n_plain = 64 * 2 * f + 64 * 2 * 64 + 128 + c * 8
    assert p4.size == n_plain + 256 + 256
    mean, var = p4[-256:-128], p4[-128:]
    assert np.abs(mean).max() > 0 and (var > 0).all() and np.abs(var - 1).max() > 0          # advanced from 0 / 1
    assert not np.array_equal(p2[-256:], p4[-256:])
    run(base[:-3] + ["--epochs", "1", "--dump-params", str(tmp_path / "p0.bin")])               # without the flag: the format of always
    assert np.fromfile(tmp_path / "p0.bin", dtype=np.float32).size == n_plain
    bad = run(base + ["--layer-norm", "--epochs", "1"], ok=False)
    assert "--batch-norm and --layer-norm exclude each other" in bad.stderr


def test_errors(pkg, orc):
    A = pkg.abi
    g = make_graph(7)

    def refused(ctx, code, **kw):
        with pytest.raises(A.GatError) as ei:
            ctx.set_batch_norm(**kw)
        assert ei.value.code == code, kw
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        for flags in (4, 8, -1):
            refused(ctx, INVALID, flags=flags)
        refused(ctx, INVALID, flags=A.BN_SKIP_LAST)              # GAT_BN_SKIP_LAST alone
        for eps in (0.0, -1e-5, float("inf"), float("nan")):
            refused(ctx, INVALID, eps=eps)
        for momentum in (-0.1, 1.5, float("inf"), float("nan")):
            refused(ctx, INVALID, momentum=momentum)
        assert ctx.param_count(A.PARAM_NORM_G) == 0              # nothing above took effect
        ctx.set_batch_norm(momentum=0.0)
        ctx.set_batch_norm(skip_last=True, momentum=1.0)         # again, while nothing sized the buffers
        assert ctx.param_count(A.PARAM_NORM_G) == 128 and ctx.param_count(A.PARAM_NORM_B) == 128
        with pytest.raises(A.GatError) as ei:                    # one normaliser per context: the second call is the one refused
            ctx.set_norm()
        assert ei.value.code == UNSUPPORTED
        ctx.set_norm(layer=False)                                # off stays allowed
        ctx.params_set(A.PARAM_NORM_B, np.ones(128, np.float32))
        refused(ctx, STATE)                                      # after gat_params_set
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.set_norm()
        refused(ctx, UNSUPPORTED)                                # the other order
        ctx.set_batch_norm(flags=0)                              # off stays allowed
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.set_graph(g["row_ptr"], g["col_idx"])
        refused(ctx, STATE)                                      # after gat_set_graph
        refused(ctx, STATE, flags=0)                             # flags == 0 too: the rule is about the call order
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.grads_get(A.PARAM_W)
        refused(ctx, STATE)                                      # after gat_grads_get
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"], flat_lrelu_index=True) as ctx:
        refused(ctx, UNSUPPORTED)
        ctx.set_batch_norm(flags=0)                              # off stays allowed


def test_shards_are_refused(pkg):
    """A shard-shaped graph (n_table != n_rows, or table_row0 != 0) is refused by the call that sets it, and gat_comm_init_* on a
    batch-norm context as the readout's is: the column statistics of a shard would need an exchange that is not built."""
    A = pkg.abi
    g = make_graph(7, n=90, e=700, F=12, C=4)
    S = pkg.shard
    plan = S.make_plan(g["row_ptr"], 2, 1)
    rp_l, ci_l = S.local_csr(plan, g["row_ptr"], g["col_idx"])
    assert plan.n_table != plan.n_rows
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as ctx:
        ctx.set_batch_norm()
        with pytest.raises(A.GatError) as ei:
            ctx.set_graph(rp_l, ci_l, n_table=plan.n_table, table_row0=plan.table_row0)
        assert ei.value.code == UNSUPPORTED
        ctx.set_graph(g["row_ptr"], g["col_idx"])                # the whole graph is taken
        ctx.set_features(g["x"]); ctx.set_labels(g["labels"])
        with pytest.raises(A.GatError) as ei:
            ctx.comm_init_host(1, 0, f"/gatv2_bn_{os.getpid()}", 1 << 20)
        assert ei.value.code == UNSUPPORTED


def test_experiment_library_refuses_batch_norm_with_gat_dbg(pkg):
    exp = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "libgatv2_hip_exp.so")
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import __graft_entry__ as entry
pkg = entry.load_package(); A = pkg.abi
ctx = pkg.GatContext([8, 8], [8, 8], 16, 4)
try:
    ctx.set_batch_norm()
except A.GatError as e:
    print("CODE", e.code)
ctx.set_batch_norm(flags=0)          # off stays allowed
print("OK")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GATV2_LIB=exp, GAT_DBG="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CODE 10004" in r.stdout and "OK" in r.stdout, r.stdout
