"""tests/optimizer_ref.py (the fp64 statement of the optimizer law, gatv2_abi.h "optimizer step on the device") held to torch on the CPU in
fp64, at 1e-12 relative, over 5 steps: torch.optim.SGD plain / with momentum / with nesterov / with weight_decay, torch.optim.Adam with
weight_decay, torch.optim.AdamW, torch.nn.utils.clip_grad_norm_.  The per-group clip is held to the formula of gat_clip's kernel.  Also
here: train_edge refuses bad values of the optimizer flags by text and exit code, before any device call."""
import os
import subprocess

import numpy as np
import pytest

import optimizer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
COUNTS = [37, 5, 12, 0, 9]            # group sizes (one empty group)
STEPS = 5
TOL = 1e-12


def _data(seed):
    rng = np.random.default_rng(seed)
    n = sum(COUNTS)
    p0 = rng.standard_normal(n)
    grads = []
    for _ in range(STEPS):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2, n)).astype(np.float32)
        g[rng.random(n) < 0.25] = 0
        grads.append(g)
    return p0, grads


def _torch_run(make, p0, grads, clip_global=None):
    import torch
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    params = [torch.nn.Parameter(torch.tensor(p0[off[k]:off[k + 1]], dtype=torch.float64)) for k in range(len(COUNTS))]
    opt = make(torch, params)
    out, norms = [], []
    for g in grads:
        for k, q in enumerate(params):
            q.grad = torch.tensor(g[off[k]:off[k + 1]].astype(np.float64))
        if clip_global is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, float(R.f32(clip_global)))))
        opt.step()
        out.append(np.concatenate([q.detach().numpy().copy() for q in params]))
    return out, norms


def _model_run(p0, grads, **cfg):
    m = R.Model(COUNTS, **cfg)
    p = p0.copy()
    out, norms = [], []
    for g in grads:
        m.step(p, g)
        out.append(p.copy())
        norms.append(m.global_norm)
    return out, norms


def _close(got, want):
    for t, (a, b) in enumerate(zip(got, want)):
        err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
        assert err <= TOL, (t + 1, err)


LR, WD, MU = 0.05, 0.01, 0.9
f = R.f32


@pytest.mark.parametrize("name,cfg,make", [
    ("sgd", dict(kind=R.SGD, lr=LR), lambda T, ps: T.optim.SGD(ps, lr=float(f(LR)))),
    ("sgd momentum", dict(kind=R.SGD, lr=LR, momentum=MU), lambda T, ps: T.optim.SGD(ps, lr=float(f(LR)), momentum=float(f(MU)))),
    ("sgd nesterov", dict(kind=R.SGD, lr=LR, momentum=MU, nesterov=True),
     lambda T, ps: T.optim.SGD(ps, lr=float(f(LR)), momentum=float(f(MU)), nesterov=True)),
    ("sgd weight decay", dict(kind=R.SGD, lr=LR, momentum=MU, weight_decay=WD),
     lambda T, ps: T.optim.SGD(ps, lr=float(f(LR)), momentum=float(f(MU)), weight_decay=float(f(WD)))),
    ("adam l2", dict(kind=R.ADAM, lr=LR, weight_decay=WD, betas=(0.9, 0.999), eps=1e-8),
     lambda T, ps: T.optim.Adam(ps, lr=float(f(LR)), betas=(float(f(0.9)), float(f(0.999))), eps=float(f(1e-8)), weight_decay=float(f(WD)))),
    ("adamw", dict(kind=R.ADAMW, lr=LR, weight_decay=WD, betas=(0.9, 0.999), eps=1e-8),
     lambda T, ps: T.optim.AdamW(ps, lr=float(f(LR)), betas=(float(f(0.9)), float(f(0.999))), eps=float(f(1e-8)), weight_decay=float(f(WD)))),
])
def test_model_matches_torch(name, cfg, make):
    p0, grads = _data(3)
    want, _ = _torch_run(make, p0, grads)
    got, _ = _model_run(p0, grads, **cfg)
    _close(got, want)


@pytest.mark.parametrize("thr", [0.5, 1e6])          # clipping in every step / never
def test_global_clip_matches_clip_grad_norm(thr):
    p0, grads = _data(4)
    want, tn = _torch_run(lambda T, ps: T.optim.SGD(ps, lr=float(f(LR)), momentum=float(f(MU))), p0, grads, clip_global=thr)
    got, mn = _model_run(p0, grads, kind=R.SGD, lr=LR, momentum=MU, clip_mode=R.CLIP_GLOBAL, clip_threshold=thr)
    _close(got, want)
    assert np.allclose(tn, mn, rtol=TOL, atol=0)
    if thr > 1e3:                                     # below the threshold: the unclipped run, value for value
        plain, _ = _model_run(p0, grads, kind=R.SGD, lr=LR, momentum=MU)
        assert all(np.array_equal(a, b) for a, b in zip(got, plain))


def test_group_clip_is_the_formula_of_gat_clip():
    """clip_scale_kernel: norm = sqrt(sumsq); scale = thr / (norm + 1e-9f) if norm > thr, else nothing is touched."""
    rng = np.random.default_rng(5)
    grads = [rng.standard_normal(c) * s for c, s in zip(COUNTS, (3.0, 0.1, 2.0, 1.0, 1e-3))]
    thr = 5.0
    c, norms, total = R.clip_factors(grads, R.CLIP_PER_GROUP, thr)
    for k, g in enumerate(grads):
        n = np.sqrt(np.sum(g * g))
        assert norms[k] == n
        want = thr / (n + np.float64(np.float32(1e-9))) if n > thr else 1.0
        assert c[k] == want
    assert [bool(x < 1) for x in c] == [True, False, True, False, False]
    assert abs(total - np.sqrt(sum(float(np.sum(g * g)) for g in grads))) <= 1e-12 * total
    cn, _, _ = R.clip_factors(grads, R.CLIP_NONE, thr)
    assert np.array_equal(cn, np.ones(len(grads)))


def test_decay_groups_mask_and_zero_entries():
    """lambda applies to the groups whose bit is set only; an entry with g = 0, lambda = 0 and zero state does not move, in any kind."""
    p0, grads = _data(6)
    still = np.zeros(sum(COUNTS), bool)
    still[40:50] = True                               # inside groups 1 and 2
    for g in grads:
        g[still] = 0
    for kind, extra in ((R.SGD, dict(momentum=MU)), (R.ADAM, {}), (R.ADAMW, {})):
        got, _ = _model_run(p0, grads, kind=kind, lr=LR, weight_decay=WD, decay_groups=[0, 4], **extra)
        assert np.array_equal(got[-1][still], p0[still])
        allg, _ = _model_run(p0, grads, kind=kind, lr=LR, weight_decay=WD, **extra)
        assert not np.array_equal(allg[-1][still], p0[still])


def _run(args):
    e = dict(os.environ)
    e.pop("DATA_ROOT", None)
    return subprocess.run([BIN, "--heads", "8,8", "--outdims", "8,8"] + args, capture_output=True, text=True, env=e, timeout=120)


@pytest.mark.parametrize("args,msg", [
    (["--weight-decay", "-1"], "Error: --weight-decay must be a finite number >= 0\n"),
    (["--weight-decay", "nan"], "Error: --weight-decay must be a finite number >= 0\n"),
    (["--weight-decay", "1e-3x"], "Error: --weight-decay must be a finite number >= 0\n"),
    (["--momentum", "1"], "Error: --momentum must be in [0, 1)\n"),
    (["--momentum", "-0.5"], "Error: --momentum must be in [0, 1)\n"),
    (["--clip-global", "0"], "Error: --clip-global must be a finite number > 0\n"),
    (["--clip-global", "inf"], "Error: --clip-global must be a finite number > 0\n"),
    (["--optimizer", "adam", "--momentum", "0.9"], "Error: --momentum needs --optimizer sgd\n"),
    (["--nesterov"], "Error: --nesterov needs --optimizer sgd and --momentum M > 0\n"),
    (["--optimizer", "adamw", "--momentum", "0.9", "--nesterov"], "Error: --momentum needs --optimizer sgd\n"),
])
def test_train_edge_refuses_bad_optimizer_flags(args, msg):
    """Refused with the message and the usage text, exit code 1, before the program looks at a device or a dataset."""
    r = _run(args)
    assert r.returncode == 1
    assert r.stderr.startswith(msg + "Usage: train_edge "), r.stderr
    assert "--weight-decay X" in r.stderr and "--fused-step" in r.stderr
    assert r.stdout == ""                             # not even the memory tracker's block: nothing touched the GPU


def test_train_edge_accepts_adamw_by_name(tmp_path):
    r = _run(["--optimizer", "adamw", "--weight-decay", "0.01", "--data-root", str(tmp_path)])
    assert "Invalid optimizer choice" not in r.stderr
    assert "  Optimizer: adamw\n" in r.stdout
