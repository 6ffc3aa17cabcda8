"""gat_clip, gat_step_sgd and gat_step_adam (gat_dense_kernels.hip: sumsq_kernel / clip_scale_kernel, sgd_kernel,
adam_kernel) against fp64, on parameter and gradient values written straight into a context (params_set / grads_set:
no graph, no model run).  The fp64 references take the hyper-parameters as the float32 values the C ABI receives."""
import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

F32 = np.float32


def _ctx(pkg, in_dim=5, c=3):
    return pkg.GatContext([8], [8], in_dim, c)              # nW = 128 in_dim, nA = 64, nWo = 8 c: 728 values by default (not a multiple of 256)


def _groups(A, ctx):
    return [(g, ctx.param_count(g)) for g in (A.PARAM_W, A.PARAM_A, A.PARAM_WO)]


def _set(ctx, groups, setter, flat):
    off = 0
    for g, n in groups:
        setter(g, flat[off:off + n])
        off += n


def _get(ctx, groups, getter):
    return np.concatenate([getter(g) for g, _ in groups])


def test_sgd(pkg):
    A = pkg.abi
    rng = np.random.default_rng(11)
    with _ctx(pkg) as ctx:
        groups = _groups(A, ctx)
        n = sum(k for _, k in groups)
        p = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(F32)
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(F32)
        zero = rng.random(n) < 0.25
        g[zero] = 0
        lr = F32(0.37)
        _set(ctx, groups, ctx.params_set, p)
        _set(ctx, groups, ctx.grads_set, g)
        ctx.step_sgd(float(lr))
        got = _get(ctx, groups, ctx.params_get)
        step = np.float64(lr) * g.astype(np.float64)
        want = p.astype(np.float64) - step
        # one rounding of the result (the product is exact inside an fma): 1 ulp of the larger operand
        ulp = np.spacing(np.maximum(np.abs(p), np.abs(step).astype(F32))).astype(np.float64)
        err = float((np.abs(got - want) / ulp).max())
        parity.record("sgd, ulp of max(|p|, |lr g|)", err, 1.0)
        assert err <= 1.0, err
        assert np.array_equal(got[zero].view(np.uint32), p[zero].view(np.uint32))     # g = 0: bit-identical
        assert np.array_equal(_get(ctx, groups, ctx.grads_get).view(np.uint32), g.view(np.uint32))   # the gradients are only read


def _adam64(p, g, m, v, lr, b1, b2, eps, t):
    m[:] = b1 * m + (1.0 - b1) * g
    v[:] = b2 * v + (1.0 - b2) * g * g
    p -= lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps)


def test_adam_five_steps(pkg):
    A = pkg.abi
    rng = np.random.default_rng(12)
    lr, b1, b2, eps = (float(F32(v)) for v in (0.01, 0.9, 0.999, 1e-8))
    with _ctx(pkg) as ctx, _ctx(pkg) as fresh:
        groups = _groups(A, ctx)
        n = sum(k for _, k in groups)
        p0 = rng.standard_normal(n).astype(F32)
        tiny = np.arange(n) % 7 == 1                        # |g| ~ 1e-10: sqrt(v_hat) << eps, eps decides the step
        still = np.arange(n) % 7 == 3                       # g = 0 in every step: p must not move
        _set(ctx, groups, ctx.params_set, p0)
        p = p0.astype(np.float64)
        m, v = np.zeros(n), np.zeros(n)
        pmax = float(np.abs(p0).max()) + 5 * 3.2 * lr
        for t in range(1, 6):
            g = (rng.standard_normal(n) * 10.0 ** rng.integers(-4, 2, n)).astype(F32)
            g[tiny] = (rng.choice([-1.0, 1.0], int(tiny.sum())) * rng.uniform(0.5e-10, 2e-10, int(tiny.sum()))).astype(F32)
            g[still] = 0
            if t == 3:                                      # the same parameters and gradient, but no history: moments are state
                _set(fresh, groups, fresh.params_set, _get(ctx, groups, ctx.params_get))
                _set(fresh, groups, fresh.grads_set, g)
                fresh.step_adam(lr, b1, b2, eps, 3)
            _set(ctx, groups, ctx.grads_set, g)
            ctx.step_adam(lr, b1, b2, eps, t)
            _adam64(p, g.astype(np.float64), m, v, lr, b1, b2, eps, t)
            got = _get(ctx, groups, ctx.params_get)
            assert np.isfinite(got).all()
            # an update is at most ~3.2 lr; fp32 powf, sqrtf and the divides give under 3e-6 of it; p itself rounds once per step
            bar = t * (1e-5 * lr + 2.0 ** -23 * pmax)
            err = float(np.abs(got - p).max())
            parity.record(f"adam t={t}", err, bar)
            assert err <= bar, (t, err, bar)
            assert np.array_equal(got[still].view(np.uint32), p0[still].view(np.uint32))
            if t == 3:
                other = _get(fresh, groups, fresh.params_get)
                moved = ~still
                assert float(np.abs(other - got)[moved].max()) > 0.1 * lr
                assert np.array_equal(other[still].view(np.uint32), p0[still].view(np.uint32))
        # the eps-dominated entries moved by ~ lr |m_hat| / eps, not by ~ lr
        d = np.abs(p - p0.astype(np.float64))[tiny]
        assert 0 < d.max() < 5 * lr * 2e-10 / eps * 1.5 and d.max() < 0.5 * lr


def test_clip_groups_independently(pkg):
    A = pkg.abi
    rng = np.random.default_rng(13)
    thr = 5.0
    results = []
    for _ in range(2):
        with _ctx(pkg, in_dim=1433) as ctx:                 # nW = 183,424: 179 strides of the single block's sum
            nW, nA, nWo = (ctx.param_count(g) for g in (A.PARAM_W, A.PARAM_A, A.PARAM_WO))
            if not results:
                gW = (rng.standard_normal(nW) * 0.1).astype(F32)       # norm ~ 42.8 > thr
                ga = (rng.standard_normal(nA) * 0.1).astype(F32)       # norm ~ 0.8 < thr
                gWo = np.zeros(nWo, F32)
                assert np.linalg.norm(gW.astype(np.float64)) > 2 * thr > 4 * np.linalg.norm(ga.astype(np.float64))
            ctx.grads_set(A.PARAM_W, gW); ctx.grads_set(A.PARAM_A, ga); ctx.grads_set(A.PARAM_WO, gWo)
            ctx.clip(1000.0)                                # nothing above the threshold: nothing is touched
            for grp, g in ((A.PARAM_W, gW), (A.PARAM_A, ga), (A.PARAM_WO, gWo)):
                assert np.array_equal(ctx.grads_get(grp).view(np.uint32), g.view(np.uint32))
            ctx.clip(thr)
            results.append([ctx.grads_get(g) for g in (A.PARAM_W, A.PARAM_A, A.PARAM_WO)])
    cW, ca, cWo = results[0]
    assert all(np.isfinite(r).all() for r in results[0])
    assert np.array_equal(ca.view(np.uint32), ga.view(np.uint32)) and np.array_equal(cWo.view(np.uint32), gWo.view(np.uint32))
    w64, c64 = gW.astype(np.float64), cW.astype(np.float64)
    err = abs(np.linalg.norm(c64) / thr - 1.0)
    parity.record("clip: |norm after / thr - 1|", err, 1e-5)
    assert err <= 1e-5, err
    s = float(c64 @ w64) / float(w64 @ w64)                 # the one scale factor, and every entry is that multiple of its old value
    dev = float((np.abs(c64 - s * w64) / np.maximum(np.abs(c64), 1e-30)).max())
    parity.record("clip: direction, relative deviation per entry", dev, 2.0 ** -23)
    assert 0 < s < 1 and dev <= 2.0 ** -23, (s, dev)
    for r0, r1 in zip(*results):                            # fixed summation order: two contexts agree bit for bit
        assert np.array_equal(r0.view(np.uint32), r1.view(np.uint32))


def test_clip_all_seven_groups(pkg):
    """test_clip_groups_independently on a context that has every parameter group: each group's gradient is a constant of its own,
    some norms above the threshold and some below; every group is clipped by its own norm (the fp64 bars of the test above), a
    group below the threshold comes back bit for bit."""
    A = pkg.abi
    thr = 5.0
    ALL = (A.PARAM_W, A.PARAM_A, A.PARAM_WO, A.PARAM_WRES, A.PARAM_B, A.PARAM_LN_G, A.PARAM_LN_B)
    with pkg.GatContext([2, 2], [4, 4], 5, 3) as ctx:
        ctx.set_residual(linear=True, bias=True)
        ctx.set_norm()
        n = 12                                              # a ring of a dozen nodes with self-loops (clip reads no graph: the context is complete)
        row_ptr = (2 * np.arange(n + 1)).astype(np.int32)
        col_idx = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1).reshape(-1).astype(np.int32)
        ctx.set_graph(row_ptr, col_idx)
        ctx.set_features(np.zeros((n, 5), F32))
        ctx.set_labels(np.zeros(n, np.int32))
        counts = [ctx.param_count(g) for g in ALL]
        assert counts == [8 * 2 * 5 + 8 * 2 * 8, 16, 12, 8 * 5 + 8 * 8, 16, 16, 16]
        # constants 3 (-1)^k / (k + 1): norms 43.3 (W), 6 (a), 7.6 (Wres) above thr = 5; 3.5 (Wo), 2.4 (b), 2 (gamma), 1.7 (beta) below
        grads = [np.full(cnt, (-1.0) ** k * 3.0 / (k + 1), F32) for k, cnt in enumerate(counts)]
        norms = [np.linalg.norm(g.astype(np.float64)) for g in grads]
        above = [nm > thr for nm in norms]
        assert above == [True, True, False, True, False, False, False] and all(abs(nm / thr - 1.0) > 0.15 for nm in norms)
        for grp, g in zip(ALL, grads):
            ctx.grads_set(grp, g)
        ctx.clip(thr)
        for k, (grp, g) in enumerate(zip(ALL, grads)):
            got = ctx.grads_get(grp)
            if not above[k]:
                assert np.array_equal(got.view(np.uint32), g.view(np.uint32)), k
                continue
            w64, c64 = g.astype(np.float64), got.astype(np.float64)
            err = abs(np.linalg.norm(c64) / thr - 1.0)
            parity.record(f"clip, seven groups, group {k}: |norm after / thr - 1|", err, 1e-5)
            assert err <= 1e-5, (k, err)
            s = float(c64 @ w64) / float(w64 @ w64)
            dev = float((np.abs(c64 - s * w64) / np.maximum(np.abs(c64), 1e-30)).max())
            parity.record(f"clip, seven groups, group {k}: direction, relative deviation per entry", dev, 2.0 ** -23)
            assert 0 < s < 1 and dev <= 2.0 ** -23, (k, s, dev)
