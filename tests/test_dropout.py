"""Attention and feature dropout on the GPU (include/gatv2_abi.h "dropout"): off is off, the mask taps against the numpy
hash, parity of every dispatcher family against an fp64 autograd model with the same masks, eval mode and the step counter,
graph replay, shards, the full Products shape, error paths."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

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
        b.set_dropout(0.0, 0.0, seed=99, first_step=4)
        ra, rb = a.step(), b.step()
        assert ra == rb
        for x, y in zip(FC.grads(pkg, a, WAWO), FC.grads(pkg, b, WAWO)):
            assert np.array_equal(x, y)
        assert b.dropout_step() == 4                         # nothing runs, nothing advances


def test_mask_taps_equal_the_numpy_hash(pkg, orc):
    A = pkg.abi
    g = make_graph(2)
    heads, outdims = [8, 4], [8, 16]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    seed = 0x1234_5678_9ABC
    with make_ctx(pkg, g, heads, outdims, orc.xavier_params(cfg, 1)) as ctx:
        ctx.set_dropout(0.4, 0.3, seed=seed, first_step=0)
        for step in (1, 2):
            ctx.step()
            assert ctx.dropout_step() == step
            for l in range(2):
                want_a = R.attn_factor(seed, step, l, g["row_ptr"], heads[l], 0.3)
                assert np.array_equal(ctx.tap(A.TAP_ATTN_KEEP, l), want_a), (step, l)
                want_f = R.feat_factor(seed, step, l, g["n"], cfg.in_dims[l], 0.4)
                assert np.array_equal(ctx.tap(A.TAP_FEAT_KEEP, l), want_f), (step, l)
        hub = slice(g["row_ptr"][7], g["row_ptr"][8])
        assert hub.stop - hub.start == 300


@pytest.mark.parametrize("pf", [0.0, 0.5])
@pytest.mark.parametrize("name,heads,outdims,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_parity_against_fp64(pkg, orc, name, heads, outdims, kw, pf):
    A = pkg.abi
    pa, seed = 0.3, 77
    g = make_graph(5, n=150, e=700)              # small enough that some Xavier seed keeps every |s|, |h_pre| off the kink
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    attn = [R.attn_factor(seed, 1, l, g["row_ptr"], heads[l], pa) for l in range(cfg.L)]
    feat = [R.feat_factor(seed, 1, l, g["n"], cfg.in_dims[l], pf) for l in range(cfg.L)] if pf > 0 else None
    bf16 = kw.get("dtype") == "bf16"
    P, ref = FC.pick_params(orc, cfg, lambda ps, P: (FC.run_model(cfg, g, P, attn=attn, feat=feat, bf16_pl=bf16),),
                            FC.CLEAR_HPRE)                   # bf16: the reference gathers the bf16-rounded table too
    ref["loss"].backward()
    tol = 1e-2 if kw.get("dtype") == "bf16" else 1e-4
    with make_ctx(pkg, g, heads, outdims, P, **kw) as ctx:
        ctx.set_dropout(pf, pa, seed=seed, first_step=0)
        loss, _ = ctx.step()
        FC.compare(pkg, ctx, g, cfg, ref, loss, tol, taps=["hpre"], groups=WAWO)
        if kw.get("keep_taps"):                  # the kept alpha is the softmax's (rows sum to 1), not kappa*s_a*alpha
            al = ctx.tap(A.TAP_ALPHA, 0)
            rp = g["row_ptr"]
            sums = np.add.reduceat(al, rp[:-1][np.diff(rp) > 0], axis=1)
            assert np.abs(sums - 1).max() < 1e-4


def test_eval_mode_and_counter(pkg, orc):
    A = pkg.abi
    g = make_graph(3)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 2)
    with make_ctx(pkg, g, [8, 8], [8, 8], P) as plain, make_ctx(pkg, g, [8, 8], [8, 8], P) as ctx:
        ctx.set_dropout(0.5, 0.5, seed=5, first_step=0)
        ctx.set_training(False)
        assert ctx.forward() == plain.forward()
        for l in range(2):
            assert np.array_equal(ctx.tap(A.TAP_HPRE, l), plain.tap(A.TAP_HPRE, l))
        assert ctx.dropout_step() == 0
        ctx.set_training(True)
        ctx.forward()
        assert ctx.dropout_step() == 1
        ctx.step()
        assert ctx.dropout_step() == 2
        ctx.step_graph(True)
        for k in range(3):                       # eager warm-up, capture + launch, replay
            ctx.step()
            assert ctx.dropout_step() == 3 + k
        ctx.step_graph(False)
        for l in range(2):                       # the phase API
            ctx.layer_project(l); ctx.layer_forward_edges(l)
        ctx.head_forward(want_loss=False); ctx.head_backward()
        for l in (1, 0):
            ctx.layer_backward_edges(l); ctx.layer_backward_dense(l)
        assert ctx.dropout_step() == 6


def test_first_step_resumes_the_sequence(pkg, orc):
    g = make_graph(4)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 2)

    def run(first, k):
        out = []
        with make_ctx(pkg, g, [8, 8], [8, 8], P) as ctx:
            ctx.set_dropout(0.5, 0.3, seed=9, first_step=first)
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
            c.set_dropout(0.5, 0.5, seed=21, first_step=0)
        r.step_graph(True)
        for _ in range(3):
            e.zero_grad(); r.zero_grad()
            assert e.step() == r.step()
            for x, y in zip(FC.grads(pkg, e, WAWO), FC.grads(pkg, r, WAWO)):
                assert np.array_equal(x, y)


def test_errors(pkg, orc):
    A = pkg.abi
    g = make_graph(7)
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    with make_ctx(pkg, g, [8, 8], [8, 8], orc.xavier_params(cfg, 1)) as ctx:
        for pf, pa in ((1.0, 0.0), (0.0, 1.0), (-0.1, 0.0), (float("nan"), 0.0), (0.0, float("nan"))):
            with pytest.raises(A.GatError) as ei:
                ctx.set_dropout(pf, pa, seed=1)
            assert ei.value.code == 10001                    # GAT_E_INVALID
        for bounds in ([0, g["n"] - 1], [0, 100, g["n"]], [1, g["n"]]):
            with pytest.raises(A.GatError):
                ctx.set_shard_bounds(bounds)
        ctx.set_shard_bounds([0, g["n"]])                    # one rank: the identity map


def test_experiment_library_refuses_dropout_with_gat_dbg(pkg):
    exp = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "libgatv2_hip_exp.so")
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import __graft_entry__ as entry
pkg = entry.load_package(); A = pkg.abi
ctx = pkg.GatContext([8, 8], [8, 8], 16, 4)
try:
    ctx.set_dropout(0.0, 0.5, seed=1)
except A.GatError as e:
    print("CODE", e.code)
ctx.set_dropout(0.0, 0.0, seed=1)          # off stays allowed
print("OK")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GATV2_LIB=exp, GAT_DBG="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CODE 10004" in r.stdout and "OK" in r.stdout, r.stdout


@pytest.mark.parametrize("ranks", [2, 3])
def test_train_edge_ranks_with_dropout(pkg, tmp_path, ranks):
    """train_edge --ranks P --transport host (ranks share the GPU; replicated layer-0 input, exchanged hidden layers): the
    shards draw the masks of one GPU, so the epochs print the same numbers and end at the same parameters."""
    ds = pkg.synth.make_dataset("cora", scale=0.15)
    pkg.synth.write_text_dataset(ds, str(tmp_path), "tiny")
    base = ["--dataset", "tiny", "--data-root", str(tmp_path), "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8",
            "--epochs", "3", "--optimizer", "sgd", "--lr", "0.001", "--seed", "5", "--dropout", "0.5", "--attn-dropout", "0.5"]
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
    # without the flags the run differs: the masks do something
    plain = subprocess.run([BIN] + base[:-4], capture_output=True, text=True, env=env, timeout=600)
    assert plain.returncode == 0 and re.findall(pat, plain.stdout) != re.findall(pat, one.stdout)


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
        outs = []
        for _ in range(2):                       # the same step twice: bitwise equal
            ctx.set_dropout(0.5, 0.5, seed=3, first_step=0)
            ctx.zero_grad()
            outs.append((ctx.step(), FC.grads(pkg, ctx, WAWO)))
        assert outs[0][0] == outs[1][0]
        assert all(np.array_equal(x, y) for x, y in zip(outs[0][1], outs[1][1]))
        keep = ctx.tap(A.TAP_ATTN_KEEP, 1)       # [H][E] of the last layer
        rate = float((keep != 0).mean())
        assert abs(rate - 0.5) < 5 * np.sqrt(0.25 / keep.size), rate
        # h_pre of 1,000 rows (the largest hub among them) against fp64 from the PL / PR taps and the keep tap
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
            want = np.zeros((8, 8))
            if b1 > b0:
                s = PL[col[b0:b1]].reshape(-1, 8, 8) + PR[r].reshape(8, 8)
                sc = (a1 * np.maximum(s, 0.01 * s)).sum(-1)                     # [deg, H]
                pe = np.exp(sc - np.maximum(sc.max(0), -1e9))
                alpha = pe / (pe.sum(0) + 1e-8)
                w = alpha * keep[:, b0:b1].T
                want = np.einsum("eh,ehk->hk", w, PL[col[b0:b1]].reshape(-1, 8, 8))
            err = max(err, float(np.abs(hpre[r] - want).max()))
            scale = max(scale, float(np.abs(want).max()))
        assert scale > 0 and err <= 1e-4 * scale, (err, scale)
    finally:
        ctx.close()
