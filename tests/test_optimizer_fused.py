"""The optimizer step on the device (gatv2_abi.h "optimizer step on the device"; csrc/gat_optimizer.hip: opt_prepare / opt_apply) against
tests/optimizer_ref.py, the fp64 statement of its law, which test_optimizer_fused_cpu.py holds to torch.  Parameter and gradient values
are written straight into a context (params_set / grads_set), as tests/test_optimizer.py does; section 5 runs the model.

Bars.  Adam kinds: test_adam_five_steps' own bar, t * (1e-5 lr + 2^-23 pmax), pmax from the fp64 model.  SGD kinds: an elementwise
rounding bound from the fp64 model's magnitudes — every fp32 operation of the chain rounds once —
    sum over steps of 8 * 2^-24 * (|p| + lr * (|g^| + lambda |p| + mu |buf|)).
Norms (hence the clip factor): 1e-5 relative to the fp64 norm, the bar of test_clip_groups_independently.  Achieved errors go through
parity.record (profiles/optimizer/achieved_errors.json is a copy)."""
import numpy as np
import pytest

import optimizer_ref as R
import parity

pytestmark = pytest.mark.gpu

F32 = np.float32
STEPS = 5
KINDS = {
    "sgd": dict(kind="sgd", lr=0.05),
    "sgd-momentum": dict(kind="sgd", lr=0.05, momentum=0.9),
    "sgd-nesterov": dict(kind="sgd", lr=0.05, momentum=0.9, nesterov=True),
    "adam": dict(kind="adam", lr=0.01),
    "adamw": dict(kind="adamw", lr=0.01),
}
CLIPS = {"none": None, "group": ("group", 5.0), "global": ("global", 5.0)}
WD = 0.01


def _three(pkg, in_dim=5):
    return pkg.GatContext([8], [8], in_dim, 3)              # W 128 in_dim, a 64, Wo 24: 728 values by default (partial blocks)


def _ten(pkg):
    ctx = pkg.GatContext([2, 2], [4, 4], 5, 3)              # every group live, 5 to 200 entries each: most blocks are short
    ctx.set_residual(linear=True, bias=True)
    ctx.set_norm()
    ctx.set_edge_dim(3)
    ctx.set_head_hidden(5)
    return ctx


def _groups(A, ctx):
    return [(g, ctx.param_count(g)) for g in A.PARAM_GROUPS_ALL]


def _set(groups, setter, flat):
    off = 0
    for g, n in groups:
        if n:
            setter(g, flat[off:off + n])
        off += n


def _get(groups, getter):
    return np.concatenate([getter(g) for g, n in groups if n] or [np.zeros(0, F32)])


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _data(groups, seed, steps=STEPS):
    """p0 and one gradient per step: mixed magnitudes, a quarter exact zeros, an eps-dominated class (|g| ~ 1e-10), a class that is zero
    in every step; every second live group scaled down so that its norm stays below the per-group threshold.
    Every gradient entry has the sign of its parameter, and |p0| >= 0.25 (an Adam kind moves an entry by at most ~3.2 lr per step, 0.16 in
    five): the Adam bar presumes that d = g^ + lambda p is formed to fp32 relative accuracy, and where the two terms cancel down to a few
    eps the law itself amplifies the rounding of c by lr eps / (|d| + eps)^2 — seen once with free signs: c g = -1.00002 lambda p,
    |d| = 27 eps, error 6 x the bar at t = 1 — so the data rule cancellation out; the SGD bound is elementwise and needs no such rule."""
    rng = np.random.default_rng(seed)
    n = sum(k for _, k in groups)
    p0 = (rng.choice([-1.0, 1.0], n) * (0.25 + np.abs(rng.standard_normal(n)))).astype(F32)
    tiny, still = np.arange(n) % 7 == 1, np.arange(n) % 7 == 3
    scale = np.ones(n)
    off, live = 0, 0
    for _, k in groups:
        if k:
            if live % 2 == 1:
                scale[off:off + k] = 1e-3
            live += 1
        off += k
    grads = []
    for _ in range(steps):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-4, 2, n) * scale
        g[rng.random(n) < 0.25] = 0
        g[tiny] = rng.choice([-1.0, 1.0], int(tiny.sum())) * rng.uniform(0.5e-10, 2e-10, int(tiny.sum()))
        g[still] = 0
        grads.append((np.abs(g) * np.sign(p0)).astype(F32))
    return p0, grads, still


def _model(A, groups, cfg, clip, wd, decay):
    mode = {None: R.CLIP_NONE, "group": R.CLIP_PER_GROUP, "global": R.CLIP_GLOBAL}[clip[0] if clip else None]
    return R.Model([k for _, k in groups], kind=A.OPT_KINDS[cfg["kind"]], lr=cfg["lr"], momentum=cfg.get("momentum", 0.0),
                   nesterov=cfg.get("nesterov", False), weight_decay=wd, decay_groups=decay, clip_mode=mode, clip_threshold=clip[1] if clip else 0.0)


def _partial_decay(A, groups):
    """the weight matrices take the decay; a, the biases and the norm parameters do not"""
    return [g for g, k in groups if k and g in (A.PARAM_W, A.PARAM_WO, A.PARAM_WRES, A.PARAM_WE, A.PARAM_HEAD_W)]


def _check_norms(name, info, model, clip):
    if clip is None:
        return
    for k, want in enumerate(model.norms):
        got = float(info["group_norms"][k])
        if want == 0:
            assert got == 0, (name, k, got)
            continue
        err = abs(got / want - 1.0)
        parity.record(f"{name}: norm of group {k}", err, 1e-5)
        assert err <= 1e-5, (name, k, got, want)
    if clip[0] == "global":
        err = abs(float(info["global_norm"]) / model.global_norm - 1.0)
        parity.record(f"{name}: global norm", err, 1e-5)
        assert err <= 1e-5, (name, info["global_norm"], model.global_norm)


def _run_case(A, ctx, name, cfg, clip, wd, decay, data, steps=STEPS):
    """`steps` optimizer steps on ctx against the fp64 model at the bars of the module docstring; returns the parameters after the last."""
    groups = _groups(A, ctx)
    p0, grads, still = data
    model = _model(A, groups, cfg, clip, wd, decay)
    ctx.set_optimizer(cfg["kind"], cfg["lr"], momentum=cfg.get("momentum", 0.0), nesterov=cfg.get("nesterov", False), weight_decay=wd,
                      decay_groups=decay, clip=clip)
    _set(groups, ctx.params_set, p0)
    p = p0.astype(np.float64)
    adam = cfg["kind"] != "sgd"
    pmax, bound = float(np.abs(p).max()), np.zeros(len(p))
    lr, lam, mu = model.lr, model.lam, model.mu
    fixed = still & (lam == 0)
    got = p0
    for t in range(1, steps + 1):
        g = grads[t - 1]
        _set(groups, ctx.grads_set, g)
        ctx.optimizer_step()
        model.step(p, g)
        got = _get(groups, ctx.params_get)
        info = ctx.optimizer_info()
        assert info["t"] == t and model.t == t
        assert np.isfinite(got).all()
        assert np.array_equal(_bits(_get(groups, ctx.grads_get)), _bits(g))          # the gradient buffer is only read
        _check_norms(f"{name} t={t}", info, model, clip)
        diff = np.abs(got - p)
        if adam:
            pmax = max(pmax, float(np.abs(p).max()))
            bar = t * (1e-5 * lr + 2.0 ** -23 * pmax)
            err = float(diff.max())
            parity.record(f"{name} t={t}", err, bar)
            assert err <= bar, (name, t, err, bar)
        else:
            bound += 8 * 2.0 ** -24 * (model.last["p"] + lr * (model.last["ghat"] + lam * model.last["p"] + mu * model.last["buf"]))
            ratio = float((diff / np.maximum(bound, 1e-300)).max())
            parity.record(f"{name} t={t}: error / elementwise rounding bound", ratio, 1.0)
            assert ratio <= 1.0, (name, t, ratio)
        assert np.array_equal(_bits(got[fixed]), _bits(p0[fixed])), (name, t)        # g = 0, no decay, zero state: bit for bit
    return got


# ---- 1. every kind x clip mode x (lambda = 0, lambda > 0 on some groups), 5 steps ------------------------------------------------------
@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", ["three", "ten"])
def test_kinds_clips_decay(pkg, shape, kind, clip):
    A = pkg.abi
    make = _three if shape == "three" else _ten
    results = {}
    for wd in (0.0, WD):
        with make(pkg) as ctx:
            groups = _groups(A, ctx)
            if shape == "ten":
                assert all(5 <= k <= 208 for _, k in groups), groups         # every group one short block
            else:
                assert sum(k for _, k in groups) == 728
            data = _data(groups, 21)
            decay = _partial_decay(A, groups) if wd else None
            results[wd] = _run_case(A, ctx, f"{shape} {kind} clip={clip} wd={wd}", KINDS[kind], CLIPS[clip], wd, decay, data)
    # a group whose decay bit is clear equals the lambda = 0 run bit for bit
    off = 0
    for g, k in groups:
        if k and g not in decay:
            assert np.array_equal(_bits(results[0.0][off:off + k]), _bits(results[WD][off:off + k])), g
        off += k
    assert not np.array_equal(_bits(results[0.0]), _bits(results[WD]))


@pytest.mark.parametrize("kind,clip", [("sgd-momentum", "global"), ("adam", "group")])
def test_many_blocks_per_group(pkg, kind, clip):
    """in_dim = 1433: 183,424 entries of W, 180 blocks whose partials one norm adds."""
    A = pkg.abi
    with _three(pkg, in_dim=1433) as ctx:
        groups = _groups(A, ctx)
        assert groups[0][1] == 183424
        _run_case(A, ctx, f"big {kind} clip={clip}", KINDS[kind], CLIPS[clip], WD, _partial_decay(A, groups), _data(groups, 22, steps=3), steps=3)


# ---- 2. exactness ------------------------------------------------------------------------------------------------------------------------
def _plain_run(pkg, make, cfg, clip, data, steps=STEPS, wd=0.0):
    A = pkg.abi
    with make(pkg) as ctx:
        groups = _groups(A, ctx)
        ctx.set_optimizer(cfg["kind"], cfg["lr"], momentum=cfg.get("momentum", 0.0), nesterov=cfg.get("nesterov", False), weight_decay=wd, clip=clip)
        _set(groups, ctx.params_set, data[0])
        for t in range(steps):
            _set(groups, ctx.grads_set, data[1][t])
            ctx.optimizer_step()
        return _get(groups, ctx.params_get)


@pytest.mark.parametrize("kind", ["sgd-nesterov", "adamw"])
def test_global_clip_below_threshold_is_no_clip_and_runs_reproduce(pkg, kind):
    A = pkg.abi
    with _ten(pkg) as ctx:
        data = _data(_groups(A, ctx), 23)
    none = _plain_run(pkg, _ten, KINDS[kind], None, data, wd=WD)
    high = _plain_run(pkg, _ten, KINDS[kind], ("global", 1e9), data, wd=WD)
    assert np.array_equal(_bits(none), _bits(high))
    low = _plain_run(pkg, _ten, KINDS[kind], ("global", 5.0), data, wd=WD)
    again = _plain_run(pkg, _ten, KINDS[kind], ("global", 5.0), data, wd=WD)
    assert np.array_equal(_bits(low), _bits(again))             # two fresh contexts agree bit for bit
    assert not np.array_equal(_bits(low), _bits(none))


# ---- 3. the device counter and lr --------------------------------------------------------------------------------------------------------
def test_lr_schedule_and_step_count(pkg):
    A = pkg.abi
    cfg = KINDS["adam"]
    sched = [0.01, 0.02, 0.02, 0.005, 0.001]
    with _three(pkg) as ctx:
        groups = _groups(A, ctx)
        p0, grads, _ = _data(groups, 24, steps=6)
        model = _model(A, groups, cfg, None, 0.0, None)
        ctx.set_optimizer("adam", sched[0])
        _set(groups, ctx.params_set, p0)
        p = p0.astype(np.float64)
        pmax, bar = float(np.abs(p).max()), 0.0
        for t in range(1, 6):
            ctx.set_lr(sched[t - 1])
            model.lr = R.f32(sched[t - 1])
            _set(groups, ctx.grads_set, grads[t - 1])
            ctx.optimizer_step()
            model.step(p, grads[t - 1])
            info = ctx.optimizer_info()
            assert info["t"] == t and info["lr"] == F32(sched[t - 1])
            pmax = max(pmax, float(np.abs(p).max()))
            bar += 1e-5 * sched[t - 1] + 2.0 ** -23 * pmax     # the Adam bar, each step at its own lr
            err = float(np.abs(_get(groups, ctx.params_get) - p).max())
            parity.record(f"lr schedule t={t}", err, bar)
            assert err <= bar, (t, err, bar)
        # the next step uses t = 8: the model at t = 8 within the bar, the model at t = 6 far outside it
        ctx.set_optimizer_step_count(7)
        assert ctx.optimizer_info()["t"] == 7
        wrong, mw = p.copy(), model.m.copy()
        vw = model.v.copy()
        R.adam(wrong, grads[5].astype(np.float64), mw, vw, model.lr, model.lam, model.b1, model.b2, model.eps, 6)
        model.t = 7
        _set(groups, ctx.grads_set, grads[5])
        ctx.optimizer_step()
        model.step(p, grads[5])
        got = _get(groups, ctx.params_get)
        assert ctx.optimizer_info()["t"] == 8
        bar += 1e-5 * sched[-1] + 2.0 ** -23 * max(pmax, float(np.abs(p).max()))
        err = float(np.abs(got - p).max())
        parity.record("step count set to 7: next step at t=8", err, bar)
        assert err <= bar, (err, bar)
        assert float(np.abs(got - wrong).max()) > 10 * bar


# ---- 4. checkpoint -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd-momentum", "adamw"])
def test_checkpoint_resumes_bitwise(pkg, kind):
    A = pkg.abi
    cfg = KINDS[kind]
    states = (A.OPT_STATE_MOMENTUM,) if cfg["kind"] == "sgd" else (A.OPT_STATE_M, A.OPT_STATE_V)
    kw = dict(momentum=cfg.get("momentum", 0.0), weight_decay=WD, clip=("global", 5.0))
    with _ten(pkg) as ctx:
        data = _data(_groups(A, ctx), 25)
    straight = _plain_run(pkg, _ten, cfg, ("global", 5.0), data, wd=WD)
    with _ten(pkg) as a, _ten(pkg) as b:
        groups = _groups(A, a)
        a.set_optimizer(cfg["kind"], cfg["lr"], **kw)
        _set(groups, a.params_set, data[0])
        for t in range(3):
            _set(groups, a.grads_set, data[1][t])
            a.optimizer_step()
        b.set_optimizer(cfg["kind"], cfg["lr"], **kw)
        _set(groups, b.params_set, _get(groups, a.params_get))
        for w in states:
            for g, k in groups:
                st = a.optimizer_state(w, g)
                assert st.size == k and np.abs(st).max() > 0
                b.set_optimizer_state(w, g, st)
        b.set_optimizer_step_count(a.optimizer_info()["t"])
        for t in range(3, 5):
            _set(groups, b.grads_set, data[1][t])
            b.optimizer_step()
        assert b.optimizer_info()["t"] == 5
        assert np.array_equal(_bits(_get(groups, b.params_get)), _bits(straight))


# ---- 5. train_step against the long form -------------------------------------------------------------------------------------------------
def _model_ctx(pkg, batch_norm=False, dropout=True):
    """40-node ring plus chords with self-loops, 2 layers of 2 heads x 4, dropout on so that the step counter matters."""
    n = 40
    src = np.concatenate([np.arange(n), (np.arange(n) + 1) % n, (np.arange(n) * 7 + 3) % n, np.arange(n)])
    dst = np.concatenate([(np.arange(n) + 1) % n, np.arange(n), np.arange(n), np.arange(n)])
    order = np.lexsort((src, dst))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int32)
    rng = np.random.default_rng(26)
    ctx = pkg.GatContext([2, 2], [4, 4], 6, 3)
    if batch_norm:
        ctx.set_batch_norm()
    if dropout:
        ctx.set_dropout(0.2, 0.2, seed=5)
    ctx.set_graph(row_ptr, src[order].astype(np.int32))
    ctx.set_features(rng.standard_normal((n, 6)).astype(F32))
    ctx.set_labels(rng.integers(0, 3, n).astype(np.int32))
    ctx.params_init(7)
    return ctx


OPT5 = dict(kind="adam", lr=0.01, weight_decay=WD, clip=("group", 0.05))


def _everything(A, ctx):
    groups = _groups(A, ctx)
    out = [_get(groups, ctx.params_get)]
    for w in (A.OPT_STATE_M, A.OPT_STATE_V):
        out.append(np.concatenate([ctx.optimizer_state(w, g) for g, k in groups if k]))
    return np.concatenate(out)


def _long_form(ctx):
    ctx.zero_grad()
    r = ctx.step()
    ctx.optimizer_step()
    return r


def test_train_step_is_the_long_form(pkg):
    A = pkg.abi
    with _model_ctx(pkg) as a, _model_ctx(pkg) as b:
        a.set_optimizer(**OPT5)
        b.set_optimizer(**OPT5)
        for i in range(4):
            ra, rb = a.train_step(), _long_form(b)
            assert _bits([ra[0]])[0] == _bits([rb[0]])[0] and ra[1] == rb[1], (i, ra, rb)
            assert np.array_equal(_bits(_everything(A, a)), _bits(_everything(A, b))), i
        assert a.dropout_step() == b.dropout_step() == 4
        assert a.optimizer_info()["t"] == 4
        assert float(np.abs(_everything(A, a)).max()) > 0


def test_train_step_replay_is_the_eager_run(pkg):
    A = pkg.abi
    with _model_ctx(pkg) as a, _model_ctx(pkg) as b:
        a.set_optimizer(**OPT5)
        b.set_optimizer(**OPT5)
        a.step_graph(True)
        states = [a.step_graph_state()]
        for i in range(6):                                   # eager, capture, 4 replays
            if i == 4:                                       # a schedule between replays: takes effect, the capture stays
                a.set_lr(0.003)
                b.set_lr(0.003)
            ra, rb = a.train_step(), _long_form(b)
            states.append(a.step_graph_state())
            assert _bits([ra[0]])[0] == _bits([rb[0]])[0] and ra[1] == rb[1], (i, ra, rb)
            assert np.array_equal(_bits(_everything(A, a)), _bits(_everything(A, b))), i
        assert states == [1, 1, 2, 2, 2, 2, 2], states
        assert a.optimizer_info()["lr"] == F32(0.003) and a.optimizer_info()["t"] == 6 and a.dropout_step() == 6
        # step() on the captured slot: dropped and re-armed, and still the eager step bit for bit
        ra, rb = a.step(), b.step()
        assert a.step_graph_state() == 1
        assert _bits([ra[0]])[0] == _bits([rb[0]])[0] and ra[1] == rb[1]
        groups = _groups(A, a)
        assert np.array_equal(_bits(_get(groups, a.grads_get)), _bits(_get(groups, b.grads_get)))
        # back to train_step: eager, capture; then other hyper-parameters drop the capture
        for i in range(2):
            ra, rb = a.train_step(), _long_form(b)
            assert np.array_equal(_bits(_everything(A, a)), _bits(_everything(A, b))), i
        assert a.step_graph_state() == 2
        changed = dict(OPT5, weight_decay=2 * WD)
        a.set_optimizer(**changed)
        b.set_optimizer(**changed)
        assert a.step_graph_state() == 1
        assert a.optimizer_info()["t"] == 8                  # the same kind: state and t are kept
        for i in range(3):
            ra, rb = a.train_step(), _long_form(b)
            assert np.array_equal(_bits(_everything(A, a)), _bits(_everything(A, b))), i
        assert a.step_graph_state() == 2


def test_train_step_replay_advances_batch_norm_once_per_call(pkg):
    A = pkg.abi
    with _model_ctx(pkg, batch_norm=True) as a, _model_ctx(pkg, batch_norm=True) as b:
        a.set_optimizer(**OPT5)
        b.set_optimizer(**OPT5)
        a.step_graph(True)
        seen = []
        for i in range(4):
            a.train_step()
            _long_form(b)
            for w in (A.BN_RUNNING_MEAN, A.BN_RUNNING_VAR):
                assert np.array_equal(_bits(a.batch_norm_stats(w)), _bits(b.batch_norm_stats(w))), (i, w)
            seen.append(a.batch_norm_stats(A.BN_RUNNING_MEAN).copy())
            assert i == 0 or not np.array_equal(seen[-1], seen[-2])
        assert a.step_graph_state() == 2
        assert np.array_equal(_bits(_everything(A, a)), _bits(_everything(A, b)))


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
BAD = [
    dict(kind=0), dict(kind=4), dict(flags=2), dict(clip=(3, 1.0)),
    dict(kind="sgd", nesterov=True), dict(kind="adam", nesterov=True, momentum=0.5), dict(kind="adamw", nesterov=True),
    dict(kind="adam", betas=(0.0, 0.999)), dict(kind="adam", betas=(0.9, 1.0)), dict(kind="adamw", betas=(float("nan"), 0.999)),
    dict(eps=-1e-8), dict(eps=float("inf")), dict(lr=-0.1), dict(lr=float("nan")), dict(weight_decay=-1.0), dict(weight_decay=float("inf")),
    dict(momentum=-0.1), dict(momentum=float("nan")), dict(momentum=1.0),
    dict(clip=("group", 0.0)), dict(clip=("global", -1.0)), dict(clip=("global", float("inf"))), dict(clip=("group", float("nan"))),
    dict(decay_groups=1 << 10), dict(decay_groups=0x7FFFFFFF),
]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_set_optimizer_refuses(pkg, bad):
    A = pkg.abi
    cfg = dict(kind="sgd", lr=0.1)
    cfg.update(bad)
    with _three(pkg) as ctx:
        with pytest.raises(A.GatError) as e:
            ctx.set_optimizer(**cfg)
        assert e.value.code == 10001 and "gat_set_optimizer" in str(e.value)
        with pytest.raises(A.GatError) as e:             # nothing was configured
            ctx.optimizer_step()
        assert e.value.code == 10002


def test_null_config_and_call_order(pkg):
    A = pkg.abi
    with _three(pkg) as ctx:
        assert ctx.lib.gat_set_optimizer(ctx._ctx, None) == 10001
        z = np.zeros(ctx.param_count(A.PARAM_A), F32)
        for call in (ctx.optimizer_step, ctx.train_step, ctx.optimizer_info, lambda: ctx.set_lr(0.1), lambda: ctx.set_optimizer_step_count(1),
                     lambda: ctx.optimizer_state(A.OPT_STATE_M, A.PARAM_A), lambda: ctx.set_optimizer_state(A.OPT_STATE_M, A.PARAM_A, z)):
            with pytest.raises(A.GatError) as e:
                call()
            assert e.value.code == 10002, e.value
    with _model_ctx(pkg) as ctx:                            # a complete context: gat_train_step still wants the optimizer first
        with pytest.raises(A.GatError) as e:
            ctx.train_step()
        assert e.value.code == 10002 and "gat_set_optimizer" in str(e.value)
    with pkg.GatContext([8], [8], 5, 3) as ctx:             # the packed sizes are final after gat_set_optimizer
        ctx.set_optimizer("sgd", 0.1)
        with pytest.raises(A.GatError) as e:
            ctx.set_residual(bias=True)
        assert e.value.code == 10002
    with _three(pkg) as ctx:
        ctx.set_optimizer("sgd", 0.1, momentum=0.9)
        for w in (A.OPT_STATE_M, A.OPT_STATE_V, 3, -1):
            with pytest.raises(A.GatError) as e:
                ctx.optimizer_state(w, A.PARAM_A)
            assert e.value.code == 10001
        assert ctx.optimizer_state(A.OPT_STATE_MOMENTUM, A.PARAM_WRES).size == 0        # a group that is off: a no-op
        with pytest.raises(A.GatError) as e:
            ctx.set_optimizer_state(A.OPT_STATE_MOMENTUM, A.PARAM_A, z[:-1])
        assert e.value.code == 10001
        ctx.set_optimizer("adam", 0.1)                      # another kind: its own zeroed state, t = 0
        with pytest.raises(A.GatError) as e:
            ctx.optimizer_state(A.OPT_STATE_MOMENTUM, A.PARAM_A)
        assert e.value.code == 10001
        assert not ctx.optimizer_state(A.OPT_STATE_V, A.PARAM_A).any() and ctx.optimizer_info()["t"] == 0
        with pytest.raises(A.GatError) as e:
            ctx.set_lr(-1.0)
        assert e.value.code == 10001


# ---- 7. the old entry points are untouched -----------------------------------------------------------------------------------------------
def test_old_entry_points_ignore_the_new_state(pkg):
    A = pkg.abi
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    with _three(pkg) as a, _three(pkg) as b:
        groups = _groups(A, a)
        p0, grads, _ = _data(groups, 27)
        b.set_optimizer("adam", 0.5, weight_decay=0.1, clip=("global", 1.0))
        for ctx in (a, b):
            _set(groups, ctx.params_set, p0)
        for t in range(1, 4):
            if t == 2:                                       # its moments and its t are its own
                _set(groups, b.grads_set, grads[4])
                keep = _get(groups, b.params_get)
                b.optimizer_step()
                _set(groups, b.params_set, keep)
            for ctx in (a, b):
                _set(groups, ctx.grads_set, grads[t - 1])
                ctx.clip(5.0)
                ctx.step_adam(lr, b1, b2, eps, t)
            assert np.array_equal(_bits(_get(groups, a.params_get)), _bits(_get(groups, b.params_get))), t
            assert np.array_equal(_bits(_get(groups, a.grads_get)), _bits(_get(groups, b.grads_get))), t
        assert b.optimizer_info()["t"] == 1
