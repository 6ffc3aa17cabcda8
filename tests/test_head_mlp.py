"""The hidden layer in front of the output head on the GPU (include/gatv2_abi.h "hidden layer"): the two row-streaming kernels through
their stateless seams (forward and gA bitwise, gradb1 within the bound of any summation order, reproducible); the whole step of every
head kind against the fp64 model of tests/head_mlp_ref.py at the project's bars (1e-4 of max-abs, 1e-2 with bf16 storage); the step
paths against each other; width 0 is a context that never made the call; the optimizer, gat_params_init, the refusals, eval_mask /
eval_rank on Z1; the train_edge host.

tests/test_head_mlp_cpu.py proves on the host that every parity case has a parameter seed clear of the kinks and of the loss clamp."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import feature_cases as FC
import head_mlp_ref as HM
import loss_ref as LR
import pair_ref as PR
import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")

E_INVALID, E_STATE, E_UNSUPPORTED = 10001, 10002, 10004
UNIT = 2.0 ** -24
F32 = np.float32
ROWS = [0, 1, 127, 128, 129, 1000]
WIDTHS = [1, 3, 4, 5, 16, 64, 65, 80, 256]
SLOPES = [0.0, 0.01]
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the seam tests need the GPU"
    return torch, torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# -- 1. the seams
@pytest.mark.parametrize("width", WIDTHS)
def test_seam_forward_is_bitwise(pkg, torch_dev, width):
    A = pkg.abi
    torch, dev = torch_dev
    rng = np.random.default_rng(500 + width)
    b1 = rng.uniform(-0.5, 0.5, width).astype(F32)
    d_b1 = torch.from_numpy(b1).to(dev)
    for rows in ROWS:
        a = rng.standard_normal((rows, width)).astype(F32)
        if rows:
            a[0, 0] = -b1[0]                                                 # a + b1 == 0 exactly: the slope branch
        for slope in SLOPES:
            d_a = torch.full((rows + 1, width), SENTINEL, device=dev)        # one row of padding behind
            d_a[:rows] = torch.from_numpy(a).to(dev)
            A.op_head_hidden_forward(d_a.data_ptr(), d_b1.data_ptr(), rows, width, slope)
            got = d_a.cpu().numpy()
            s = a + b1                                                       # np.float32: one rounding per entry
            want = np.where(s > 0, s, F32(slope) * s)
            assert np.array_equal(bits(got[:rows]), bits(want)), (rows, slope)
            assert np.all(got[rows] == SENTINEL), (rows, slope)
    assert np.array_equal(d_b1.cpu().numpy(), b1)


@pytest.mark.parametrize("width", WIDTHS)
def test_seam_backward_bitwise_and_within_the_summation_bound(pkg, torch_dev, width):
    A = pkg.abi
    torch, dev = torch_dev
    rng = np.random.default_rng(600 + width)
    for rows in ROWS:
        gz = rng.standard_normal((rows, width)).astype(F32)
        z1 = rng.standard_normal((rows, width)).astype(F32)
        z1[rng.random((rows, width)) < 0.1] = 0.0                            # Z1 == 0: the slope branch
        d_z1 = torch.from_numpy(z1).to(dev)
        for slope in SLOPES:
            want = gz * np.where(z1 > 0, F32(1.0), F32(slope))              # the fp32 product
            col64 = want.astype(np.float64).sum(0)
            bound = rows * UNIT * np.abs(want.astype(np.float64)).sum(0)     # any order of a rows-term fp32 sum
            runs = []
            for _ in range(2):
                d_gz = torch.full((rows + 1, width), SENTINEL, device=dev)
                d_gz[:rows] = torch.from_numpy(gz).to(dev)
                d_gb = torch.zeros((width + 1,), device=dev)                 # one float of padding behind
                d_gb[width] = SENTINEL
                A.op_head_hidden_backward(d_gz.data_ptr(), d_z1.data_ptr(), rows, width, slope, d_gb.data_ptr())
                runs.append((d_gz.cpu().numpy(), d_gb.cpu().numpy()))
            ga, gb = runs[0]
            assert np.array_equal(bits(ga[:rows]), bits(want)), (rows, slope)
            assert np.all(ga[rows] == SENTINEL) and gb[width] == SENTINEL, (rows, slope)
            assert np.array_equal(bits(runs[0][1]), bits(runs[1][1])), (rows, slope, "gradb1 not reproducible")
            if rows == 0:
                assert np.all(gb[:width] == 0)                               # nothing launched, nothing written
                continue
            err = np.abs(gb[:width].astype(np.float64) - col64)
            assert np.all(err <= bound), (rows, slope, float((err - bound).max()))
            parity.record(f"seam gradb1 rows{rows} w{width} s{slope} err/bound", float((err / np.maximum(bound, 1e-300)).max()), 1.0)
            # the column sums are ADDED into gradb1: from 0.5 the result is 0.5 + the sums, up to the roundings of those adds
            d_gz = torch.from_numpy(gz).to(dev)
            d_gb = torch.full((width,), 0.5, device=dev)
            A.op_head_hidden_backward(d_gz.data_ptr(), d_z1.data_ptr(), rows, width, slope, d_gb.data_ptr())
            acc = d_gb.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(acc - 0.5 - gb[:width]) <= bound + 2 * UNIT * (0.5 + np.abs(col64))), (rows, slope)
            # without a gradb1 pointer the column sums are not formed and gA is the same
            d_gz = torch.from_numpy(gz).to(dev)
            A.op_head_hidden_backward(d_gz.data_ptr(), d_z1.data_ptr(), rows, width, slope, 0)
            assert np.array_equal(bits(d_gz.cpu().numpy()), bits(want))
        assert np.array_equal(d_z1.cpu().numpy(), z1)                        # Z1 is only read


def test_seams_refuse_bad_arguments(pkg, torch_dev):
    A = pkg.abi
    torch, dev = torch_dev
    d_a = torch.full((8, 4), SENTINEL, device=dev); d_b = torch.full((4,), SENTINEL, device=dev); d_z = torch.ones((8, 4), device=dev)
    calls = [lambda: A.op_head_hidden_forward(d_a.data_ptr(), d_b.data_ptr(), -1, 4, 0.0),
             lambda: A.op_head_hidden_forward(d_a.data_ptr(), d_b.data_ptr(), 8, 0, 0.0),
             lambda: A.op_head_hidden_forward(d_a.data_ptr(), d_b.data_ptr(), 8, 4, -0.5),
             lambda: A.op_head_hidden_forward(d_a.data_ptr(), d_b.data_ptr(), 8, 4, float("nan")),
             lambda: A.op_head_hidden_forward(0, d_b.data_ptr(), 8, 4, 0.0),
             lambda: A.op_head_hidden_forward(d_a.data_ptr(), 0, 8, 4, 0.0),
             lambda: A.op_head_hidden_backward(d_a.data_ptr(), d_z.data_ptr(), -1, 4, 0.0, d_b.data_ptr()),
             lambda: A.op_head_hidden_backward(d_a.data_ptr(), d_z.data_ptr(), 8, -4, 0.0, d_b.data_ptr()),
             lambda: A.op_head_hidden_backward(d_a.data_ptr(), d_z.data_ptr(), 8, 4, 1.5, d_b.data_ptr()),
             lambda: A.op_head_hidden_backward(0, d_z.data_ptr(), 8, 4, 0.0, d_b.data_ptr()),
             lambda: A.op_head_hidden_backward(d_a.data_ptr(), 0, 8, 4, 0.0, d_b.data_ptr())]
    for call in calls:
        with pytest.raises(A.GatError) as ei:
            call()
        assert ei.value.code == E_INVALID, str(ei.value)
    torch.cuda.synchronize()
    assert torch.all(d_a == SENTINEL).item() and torch.all(d_b == SENTINEL).item()          # nothing was written
    A.op_head_hidden_forward(0, 0, 0, 4, 0.0)                                # rows == 0 launches nothing and succeeds
    A.op_head_hidden_backward(0, 0, 0, 4, 0.0, 0)


# -- 2. the whole step against the fp64 model
def compare_all(pkg, ctx, ci, ref, loss, tol):
    """loss per row, GAT_TAP_HEAD_HIDDEN, GAT_TAP_Y, hout and G of every layer, all ten gradient groups."""
    A = pkg.abi
    FC.compare(pkg, ctx, dict(ci["g"], n=HM.loss_rows(ci)), ci["cfg"], ref, loss, tol, ["hout", "G"], FC.GROUPS[:7])
    parity.check_rel("Z1", ctx.tap(A.TAP_HEAD_HIDDEN, ci["cfg"].L - 1), ref["z1"].detach().numpy(), tol)
    parity.check_abs("y", ctx.tap(A.TAP_Y), ref["y"], tol)
    for grp, name in ((A.PARAM_WE, "We"), (A.PARAM_HEAD_W, "W1"), (A.PARAM_HEAD_B, "b1")):
        got = ctx.grads_get(grp)
        if ref[name] is None:
            assert got.size == 0, name
        else:
            want = ref[name].grad.numpy().reshape(-1)
            assert got.shape == want.shape and np.abs(want).max() > 0, name
            parity.check_rel(f"grad {name}", got, want, tol)


CASES = HM.cases()


@pytest.mark.parametrize("case", CASES, ids=[HM.case_id(c) for c in CASES])
def test_step_against_fp64(pkg, orc, case):
    ci = HM.case_inputs(case)
    ref = HM.model_of(ci)
    tol = 1e-2 if ci["bf16"] else 1e-4
    with HM.make_ctx(pkg, ci) as ctx:
        assert ctx.head_hidden_info() == (ci["dh"], pkg.abi.HEAD_ACTS[ci["act"]]) and ctx.head_rows == ci["rows"]
        assert ctx.param_count(pkg.abi.PARAM_WO) == ci["g"]["c"] * ci["dh"]
        loss, correct = ctx.step()
        compare_all(pkg, ctx, ci, ref, loss, tol)
        if ci["loss"] == HM.SOFTMAX and not ci["bf16"]:
            keep = np.ones(ci["rows"], bool) if ci["mask"] is None else ci["mask"]
            assert correct == int(((np.argmax(ref["y"], axis=1) == ci["sup"]) & keep).sum())


def test_achieved_errors_are_written():
    """The errors recorded above go to the session's parity record (tests/parity.py; profiles/head_mlp/achieved_errors.json is a copy)."""
    parity.flush()


# -- 3. identities
def all_grads(A, c):
    return [c.grads_get(k) for k in A.PARAM_GROUPS_ALL]


def run_paths(pkg, ci):
    """(loss, correct), gradients and Z1 of gat_step, gat_forward + gat_backward, the phase API and three steps under gat_step_graph."""
    A = pkg.abi
    L = ci["cfg"].L
    out = {}
    with HM.make_ctx(pkg, ci) as s1, HM.make_ctx(pkg, ci) as fb, HM.make_ctx(pkg, ci) as ph, HM.make_ctx(pkg, ci) as gr:
        out["step"] = (s1.step(), all_grads(A, s1), s1.tap(A.TAP_HEAD_HIDDEN, L - 1))
        lf = fb.forward(); fb.backward()
        out["fwd_bwd"] = (lf, all_grads(A, fb), fb.tap(A.TAP_HEAD_HIDDEN, L - 1))
        for l in range(L):
            ph.layer_project(l); ph.layer_forward_edges(l)
        lp = ph.head_forward()
        ph.head_backward()
        for l in range(L - 1, -1, -1):
            ph.layer_backward_edges(l); ph.layer_backward_dense(l)
        out["phases"] = (lp, all_grads(A, ph), ph.tap(A.TAP_HEAD_HIDDEN, L - 1))
        gr.step_graph(True)
        out["replays"] = []
        for _ in range(3):                                                   # eager warm-up, capture + replay, replay
            gr.zero_grad()
            out["replays"].append((gr.step(), all_grads(A, gr), gr.tap(A.TAP_HEAD_HIDDEN, L - 1)))
        assert gr.step_graph_state() == 2
    return out


@pytest.mark.parametrize("kind", HM.KINDS)
def test_paths_agree_bitwise(pkg, orc, kind):
    """Dh = 24: the head runs its any-shape forward and backward kernels on every path, so gat_step, gat_forward + gat_backward, the
    phase API and a captured replay (three steps) agree in every bit: loss, correct, Z1 and all ten gradient groups."""
    A = pkg.abi
    ci = HM.case_inputs(("records_d8", "plain", kind, HM.SOFTMAX, 24, "relu"))
    out = run_paths(pkg, ci)
    l1, g1, z1 = out["step"]
    for name in ("fwd_bwd", "phases"):
        l, g, z = out[name]
        assert l == l1, name
        assert np.array_equal(bits(z), bits(z1)), name
        for k in A.PARAM_GROUPS_ALL:
            assert np.array_equal(bits(g[k]), bits(g1[k])), (name, k)
    for l, g, z in out["replays"]:
        assert l == l1 and np.array_equal(bits(z), bits(z1))
        for k in A.PARAM_GROUPS_ALL:
            assert np.array_equal(bits(g[k]), bits(g1[k])), ("replay", k)


def test_paths_agree_with_the_fused_head_step(pkg, orc):
    """Dh = 16 selects the head's fused step kernel in gat_step and its two-kernel form elsewhere, as D_last = 8 does without the
    feature (tests/test_pair_head.py): gradWo and the loss at 1e-5 between those two (another summation order of the same terms),
    everything else — the two new groups included — bitwise; a replay is bitwise the eager step."""
    A = pkg.abi
    ci = HM.case_inputs(("records_d8", "plain", "pair_mul", HM.SOFTMAX, 16, "relu"))
    out = run_paths(pkg, ci)
    l1, g1, z1 = out["step"]
    lf, gf, zf = out["fwd_bwd"]
    lp, gp, zp = out["phases"]
    assert lf == lp and lf[1] == l1[1] and abs(lf[0] - l1[0]) <= 1e-5 * abs(l1[0])
    assert np.array_equal(bits(zf), bits(z1)) and np.array_equal(bits(zp), bits(z1))
    for k in A.PARAM_GROUPS_ALL:
        assert np.array_equal(bits(gf[k]), bits(gp[k])), k
        if k == A.PARAM_WO:
            assert parity.rel_err(gf[k], g1[k]) <= 1e-5
        else:
            assert np.array_equal(bits(gf[k]), bits(g1[k])), k
    for l, g, z in out["replays"]:
        assert l == l1
        for k in A.PARAM_GROUPS_ALL:
            assert np.array_equal(bits(g[k]), bits(g1[k])), ("replay", k)


@pytest.mark.parametrize("kind", ["node", "pair_mul"])
def test_width_zero_is_a_context_that_never_made_the_call(pkg, orc, kind):
    A = pkg.abi
    ci = HM.case_inputs(("records_d8", "plain", kind, HM.SOFTMAX, 16, "relu"))
    g = ci["g"]
    with HM.make_ctx(pkg, ci, width=False, collect_timing=True) as a, HM.make_ctx(pkg, ci, width=0, collect_timing=True) as b:
        assert b.head_hidden_info() == (0, 0) and b.param_count(A.PARAM_HEAD_W) == 0 and b.param_count(A.PARAM_HEAD_B) == 0
        assert a.n_params == b.n_params and a.param_count(A.PARAM_WO) == g["c"] * 8
        for c in (a, b):
            c.kernel_stats_reset()
        assert a.step() == b.step()
        for k in A.PARAM_GROUPS_ALL:
            assert np.array_equal(bits(a.grads_get(k)), bits(b.grads_get(k))), k
        for tap in (A.TAP_HOUT, A.TAP_Y, A.TAP_G):
            assert np.array_equal(bits(a.tap(tap, 1)), bits(b.tap(tap, 1)))
        sa, sb = a.kernel_stats(), b.kernel_stats()
        assert {k: v[0] for k, v in sa.items()} == {k: v[0] for k, v in sb.items()}      # the same launches, class by class
        assert a.algorithmic_bytes() == b.algorithmic_bytes()
        with pytest.raises(A.GatError) as ei:
            b.tap(A.TAP_HEAD_HIDDEN, 1)
        assert ei.value.code == E_STATE
        _, pa = a.algorithmic_bytes()
    with HM.make_ctx(pkg, ci) as r:                                          # on: the documented terms
        _, pr = r.algorithmic_bytes()
        R, DL, Dh, Cn = ci["rows"], 8, 16, g["c"]
        head = 4.0 * R * (Dh + 2.0 * Cn + 2.0)
        assert pa["head_forward"] == 4.0 * R * (DL + 2.0 * Cn + 2.0)
        assert pr["head_forward"] == head + 4.0 * (R * DL + Dh * DL + 3 * R * Dh)
        assert pr["head_backward"] == head + 4.0 * (3 * R * Dh + (R * Dh + R * DL + Dh * DL) + (R * Dh + Dh * DL + R * DL))
        assert all(pr[k] == pa[k] for k in pa if k not in ("head_forward", "head_backward"))


def test_replacing_and_resampling_the_pairs_under_replay(pkg, orc):
    """After a replacing gat_set_pairs and after gat_resample_negatives a replayed step equals an eager one on a fresh context with the
    same lists: the stage's buffers keep their addresses and sizes."""
    A = pkg.abi
    ci = HM.case_inputs(("records_d8", "plain", "pair_mul", HM.SOFTMAX, 16, "relu"))
    n = ci["g"]["n"]
    u2, v2 = PR.pair_list(n, seed=99, hub=12)
    assert len(u2) == len(ci["u"])
    with HM.make_ctx(pkg, ci, u=u2, v=v2) as fresh, HM.make_ctx(pkg, ci) as cap:
        want = fresh.step(); gw = all_grads(A, fresh)
        cap.step_graph(True)
        for _ in range(3):
            cap.zero_grad()
            cap.step()
        cap.set_pairs("mul", u2, v2)                                         # re-arms: eager, capture + replay, replay on the new pairs
        for i in range(3):
            cap.zero_grad()
            assert cap.step() == want, i
            for k in A.PARAM_GROUPS_ALL:
                assert np.array_equal(bits(cap.grads_get(k)), bits(gw[k])), (i, k)
        assert cap.step_graph_state() == 2
        first = len(u2) // 2
        cap.set_negative_sampling("uniform", first=first, count=len(u2) - first, seed=5)
        cap.resample_negatives(3)
        u3, v3 = cap.pairs()
        assert np.array_equal(u3[:first], u2[:first]) and not np.array_equal(u3[first:], u2[first:])
        outs = []
        for _ in range(3):
            cap.zero_grad()
            outs.append((cap.step(), all_grads(A, cap)))
    with HM.make_ctx(pkg, ci, u=u3, v=v3) as fresh3:
        want3 = fresh3.step(); g3 = all_grads(A, fresh3)
    for l, g in outs:
        assert l == want3
        for k in A.PARAM_GROUPS_ALL:
            assert np.array_equal(bits(g[k]), bits(g3[k])), k


# -- 4. the optimizer on the new groups
def test_optimizer_covers_the_new_groups(pkg):
    """gat_clip, one SGD and two Adam steps with the bars of tests/test_optimizer.py, on the two new groups (and Wo at its new size)."""
    A = pkg.abi
    rng = np.random.default_rng(21)
    NEW = (A.PARAM_WO, A.PARAM_HEAD_W, A.PARAM_HEAD_B)
    with pkg.GatContext([2, 2], [4, 4], 5, 3) as ctx:
        ctx.set_head_hidden(40, "lrelu")
        n = 12
        row_ptr = (2 * np.arange(n + 1)).astype(np.int32)
        col_idx = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1).reshape(-1).astype(np.int32)
        ctx.set_graph(row_ptr, col_idx); ctx.set_features(np.zeros((n, 5), F32)); ctx.set_labels(np.zeros(n, np.int32))
        counts = [ctx.param_count(g) for g in NEW]
        assert counts == [3 * 40, 40 * 4, 40] and ctx.n_params == sum(ctx.param_count(g) for g in A.PARAM_GROUPS_ALL)
        ptr, cnt = ctx.grads_device()
        assert cnt == ctx.n_params
        # clip: W1's norm above the threshold, b1's and Wo's below — each group by its own norm
        thr = 5.0
        grads = [np.full(counts[0], 0.1, F32), (rng.standard_normal(counts[1]) * 2.0).astype(F32), np.full(counts[2], -0.3, F32)]
        assert np.linalg.norm(grads[1].astype(np.float64)) > 2 * thr
        for grp, g in zip(NEW, grads):
            ctx.grads_set(grp, g)
        ctx.clip(thr)
        got = [ctx.grads_get(g) for g in NEW]
        assert np.array_equal(bits(got[0]), bits(grads[0])) and np.array_equal(bits(got[2]), bits(grads[2]))
        w64, c64 = grads[1].astype(np.float64), got[1].astype(np.float64)
        err = abs(np.linalg.norm(c64) / thr - 1.0)
        parity.record("clip W1: |norm after / thr - 1|", err, 1e-5)
        assert err <= 1e-5
        s = float(c64 @ w64) / float(w64 @ w64)
        assert 0 < s < 1 and float((np.abs(c64 - s * w64) / np.maximum(np.abs(c64), 1e-30)).max()) <= 2.0 ** -23
        # SGD: one rounding of the result
        lr = F32(0.37)
        p = [(rng.standard_normal(c) * 10.0 ** rng.integers(-3, 3, c)).astype(F32) for c in counts]
        g = [(rng.standard_normal(c) * 10.0 ** rng.integers(-3, 3, c)).astype(F32) for c in counts]
        ctx.zero_grad()
        for grp, pv, gv in zip(NEW, p, g):
            ctx.params_set(grp, pv); ctx.grads_set(grp, gv)
        ctx.step_sgd(float(lr))
        for grp, pv, gv in zip(NEW, p, g):
            step = np.float64(lr) * gv.astype(np.float64)
            want = pv.astype(np.float64) - step
            ulp = np.spacing(np.maximum(np.abs(pv), np.abs(step).astype(F32))).astype(np.float64)
            err = float((np.abs(ctx.params_get(grp) - want) / ulp).max())
            parity.record(f"sgd group {grp}, ulp", err, 1.0)
            assert err <= 1.0, (grp, err)
        # Adam, two steps, moments included
        lr, b1, b2, eps = (float(F32(v)) for v in (0.01, 0.9, 0.999, 1e-8))
        p0 = [rng.standard_normal(c).astype(F32) for c in counts]
        for grp, pv in zip(NEW, p0):
            ctx.params_set(grp, pv)
        p64 = [pv.astype(np.float64) for pv in p0]
        m = [np.zeros(c) for c in counts]; v = [np.zeros(c) for c in counts]
        pmax = max(float(np.abs(pv).max()) for pv in p0) + 2 * 3.2 * lr
        for t in (1, 2):
            ctx.zero_grad()
            for k, grp in enumerate(NEW):
                gk = (rng.standard_normal(counts[k]) * 10.0 ** rng.integers(-4, 2, counts[k])).astype(F32)
                ctx.grads_set(grp, gk)
                FC.adam64(p64[k], gk.astype(np.float64), m[k], v[k], lr, b1, b2, eps, t)
            ctx.step_adam(lr, b1, b2, eps, t)
            bar = t * (1e-5 * lr + 2.0 ** -23 * pmax)
            for k, grp in enumerate(NEW):
                err = float(np.abs(ctx.params_get(grp) - p64[k]).max())
                parity.record(f"adam t={t} group {grp}", err, bar)
                assert err <= bar, (t, grp, err, bar)
        ctx.zero_grad()
        assert all(not ctx.grads_get(g).any() for g in A.PARAM_GROUPS_ALL)


# -- 5. gat_params_init
def test_params_init(pkg):
    A = pkg.abi
    g = FC.parity_graph()
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as plain, pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as hid:
        hid.set_head_hidden(24)
        for c in (plain, hid):
            c.params_init(9)
        for grp in (A.PARAM_W, A.PARAM_A):
            assert np.array_equal(bits(plain.params_get(grp)), bits(hid.params_get(grp))), grp
        Wo, W1, b1 = hid.params_get(A.PARAM_WO), hid.params_get(A.PARAM_HEAD_W), hid.params_get(A.PARAM_HEAD_B)
        assert Wo.size == g["c"] * 24 and W1.size == 24 * 8 and b1.size == 24
        lim = np.sqrt(6.0 / (8 + 24))
        assert W1.max() <= F32(lim) * (1 + 2.0 ** -22) and W1.min() > -lim and np.unique(W1).size > W1.size // 2
        limo = np.sqrt(6.0 / (g["c"] + 24))
        assert np.abs(Wo).max() <= limo * (1 + 2.0 ** -22) and np.unique(Wo).size > Wo.size // 2
        assert np.all(b1 == 0)
        again = pkg.GatContext([8, 8], [8, 8], g["f"], g["c"])
        again.set_head_hidden(24)
        again.params_init(9)
        assert np.array_equal(bits(again.params_get(A.PARAM_HEAD_W)), bits(W1))          # a function of the seed
        again.close()


# -- 6. states and refusals, the evaluations
def refused(A, code, fn, *texts):
    with pytest.raises(A.GatError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for t in texts:
        assert t in str(ei.value), str(ei.value)


def test_state_and_refusal_matrix(pkg, orc):
    A = pkg.abi
    g = FC.parity_graph()
    n = g["n"]
    new = lambda c=None, **kw: pkg.GatContext([8, 8], [8, 8], g["f"], g["c"] if c is None else c, **kw)
    with new() as c:
        refused(A, E_INVALID, lambda: c.set_head_hidden(-1), "width")
        refused(A, E_INVALID, lambda: c.set_head_hidden(16, 2), "flag")
        refused(A, E_INVALID, lambda: c.set_head_hidden(0, 4), "flag")
        c.set_head_hidden(0)
        assert c.head_hidden_info() == (0, 0)
        refused(A, E_UNSUPPORTED, lambda: c.set_head_hidden(2048 // g["c"] + 1), f"width {2048 // g['c'] + 1}", "2048")
        assert c.head_hidden_info() == (0, 0)                                # nothing stuck
        c.set_head_hidden(16, "lrelu")
        assert c.head_hidden_info() == (16, A.HEAD_ACT_LRELU)
        c.set_head_hidden(0)                                                 # back off before the layout is fixed
        assert c.head_hidden_info() == (0, 0) and c.param_count(A.PARAM_HEAD_W) == 0
        c.set_head_hidden(16)
        c.set_graph(g["row_ptr"], g["col_idx"])
        refused(A, E_STATE, lambda: c.set_head_hidden(8), "before the first")
        refused(A, E_UNSUPPORTED, lambda: c.comm_init_host(1, 0, "/gat_hidden_refused", 1 << 20), "hidden")
    with new() as c:                                                         # the state rule of gat_set_residual
        c.params_init(1)
        refused(A, E_STATE, lambda: c.set_head_hidden(16), "before the first")
        c.set_head_hidden(0)                                                 # width 0 stays a no-op
    with new() as c:
        c.grads_device()
        refused(A, E_STATE, lambda: c.set_head_hidden(16), "before the first")
    with new(flat_lrelu_index=True) as c:
        refused(A, E_UNSUPPORTED, lambda: c.set_head_hidden(16), "flat_lrelu_index")
    with new() as c:                                                         # a destination-range shard
        c.set_head_hidden(16)
        refused(A, E_UNSUPPORTED, lambda: c.set_graph(g["row_ptr"], g["col_idx"], n_table=2 * n, table_row0=0), "shard")
    with new(c=8) as c:                                                      # the LDS tile: known once the loss mode is, at the completing call
        c.set_head_hidden(256)                                               # 8 * 256 <= 2048, but 32 rows of the softmax head's backward tile
        c.set_graph(g["row_ptr"], g["col_idx"]); c.set_features(g["x"])      # (9 + 2 * 256 floats each) do not fit 60 KiB beside Wo
        refused(A, E_UNSUPPORTED, lambda: c.set_labels(g["labels"]), "width 256", "LDS")


def test_experiment_library_refuses_gat_dbg():
    """The experiment library with GAT_DBG set has no hidden-head form: GAT_E_UNSUPPORTED (a child process: the switch is read at load)."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import __graft_entry__ as e\n"
            "pkg = e.load_package(); A = pkg.abi\n"
            "c = pkg.GatContext([8, 8], [8, 8], 12, 3)\n"
            "c.set_head_hidden(0)\n"
            "try:\n    c.set_head_hidden(16)\nexcept A.GatError as ex:\n    print('CODE', ex.code, ex)\n" % (ROOT, os.path.join(ROOT, "tests")))
    exp = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "libgatv2_hip_exp.so")
    assert os.path.exists(exp), "build() makes the experiment library"
    env = dict(os.environ, GATV2_LIB=exp, GAT_DBG="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and f"CODE {E_UNSUPPORTED}" in r.stdout and "GAT_DBG" in r.stdout, r.stdout + r.stderr


def test_eval_mask_and_eval_rank_run_on_z1(pkg, orc):
    """gat_eval_mask / gat_eval_rank of a hidden-head context equal the numpy law on tap(GAT_TAP_Y), after a fused head step too."""
    import rank_ref as RK
    A = pkg.abi
    rng = np.random.default_rng(8)
    ci = HM.case_inputs(("records_d8", "plain", "pair_mul", HM.SOFTMAX, 16, "relu"))
    R = ci["rows"]
    with HM.make_ctx(pkg, ci) as ctx:
        ctx.step()                                                           # the fused head step: the evaluations re-run the head on Z1
        y = ctx.tap(A.TAP_Y).astype(np.float64)
        for mask in (np.ones(R, bool), rng.random(R) > 0.7):
            loss, correct, count = ctx.eval_mask(mask)
            lab = ci["sup"]
            want = -np.log(np.maximum(y[np.arange(R), lab], 1e-12))[mask].sum()
            assert count == int(mask.sum()) and correct == int(((np.argmax(y, 1) == lab) & mask).sum())
            assert abs(loss - want) / mask.sum() < 1e-5
    cb = HM.case_inputs(("records_d8", "plain", "pair_mul", HM.BCE, 80, "relu"))
    R = cb["rows"]
    with HM.make_ctx(pkg, cb) as ctx:
        ctx.step()
        y = ctx.tap(A.TAP_Y)
        val = rng.random(R) > 0.5
        RK.assert_same(ctx.eval_rank(val, ks=(1, 10)), RK.rank_stats(y, targets=cb["sup"], mask=val, ks=(1, 10)), "hidden head")
        loss, correct, count = ctx.eval_mask(val)
        ref = LR.head_ref(ctx.tap(A.TAP_HEAD_HIDDEN, 1), ctx.params_get(A.PARAM_WO), cb["sup"], val, HM.BCE)
        assert count == int(val.sum()) and abs(loss - ref.l.sum()) / val.sum() < 1e-4


# -- 7. the host program
def test_train_edge_head_hidden(pkg, orc):
    """train_edge --pairs mul --loss bce --head-hidden 16 on a dataset folder written here runs two epochs; --dump-params then
    --load-params reproduces the first epoch's loss bitwise (W1 and b1 travel behind We)."""
    assert os.path.exists(BIN), "build() makes the host binary"
    g = FC.host_graph(3)
    u, v, t = pkg.synth.link_pairs(g["row_ptr"], g["col_idx"], 60, 60, seed=2)
    P = len(u)
    with tempfile.TemporaryDirectory() as root:
        d = os.path.join(root, "tiny")
        os.makedirs(d)
        np.savetxt(os.path.join(d, "row_ptr.txt"), g["row_ptr"], fmt="%d")
        np.savetxt(os.path.join(d, "col_idx.txt"), g["col_idx"], fmt="%d")
        np.savetxt(os.path.join(d, "features.txt"), g["x"], fmt="%.9g")
        np.savetxt(os.path.join(d, "targets.txt"), t, fmt="%.9g")
        np.savetxt(os.path.join(d, "pairs.txt"), np.stack([u, v], 1), fmt="%d")
        env = dict(os.environ)
        env.pop("DATA_ROOT", None)
        base = [BIN, "--dataset", "tiny", "--data-root", root, "--optimizer", "adam", "--lr", "0.01", "--num-layers", "2", "--heads", "8,8",
                "--outdims", "8,8", "--pairs", "mul", "--loss", "bce", "--head-hidden", "16"]
        p0, p1 = os.path.join(root, "p0.bin"), os.path.join(root, "p1.bin")
        runs = []
        for extra in (["--epochs", "0", "--seed", "7", "--dump-params", p0], ["--epochs", "2", "--seed", "7"],
                      ["--epochs", "1", "--seed", "99", "--load-params", p0, "--dump-params", p1]):
            r = subprocess.run(base + extra, capture_output=True, text=True, env=env, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            runs.append(re.findall(r"Avg Loss: ([0-9.]+), Accuracy: ([0-9.]+)%", r.stdout))
        assert len(runs[1]) == 2 and len(runs[2]) == 1
        assert runs[2][0] == runs[1][0]                                      # the loaded parameters, not seed 99's
        n_plain = 64 * 2 * g["f"] + 64 * 2 * 64 + 64 + 64
        assert os.path.getsize(p0) == 4 * (n_plain + 1 * 16 + 16 * 8 + 16)   # W, a, Wo [1][16], W1 [16][8], b1 [16]
        a0 = np.fromfile(p0, F32)
        assert np.all(a0[-16:] == 0) and np.abs(a0[-16 - 128:-16]).max() > 0  # b1 = 0, W1 drawn
