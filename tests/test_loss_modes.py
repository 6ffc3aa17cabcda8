"""The BCE / MSE output heads on the GPU (include/gatv2_abi.h "loss modes of the output head"): the whole step of every dispatcher family
against the fp64 model of tests/loss_ref.py at the project's bars (parity.TOL absolute on y and on loss / contributing entries,
parity.GTOL of max-abs on every gradient tensor, 1e-2 with bf16 storage); the head alone against the numpy reference on its own tapped
inputs over the (C, D_last, rows) sweep; missing entries; saturation; the step paths against each other, bitwise; mode 0 is the
parent; readout; optimizers; two shards; the state and argument rules; the train_edge host.

tests/test_loss_modes_cpu.py proves on the host that every whole-step case has a parameter seed clear of the LeakyReLU kinks, few
undecided BCE entries and gradients above readout_ref.GRAD_MIN."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import feature_cases as FC
import head_cases as HC
import loss_ref as LR
import parity
import readout_ref as RR
import shard_cases
from parity import GTOL, TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
E_INVALID, E_STATE, E_UNSUPPORTED = 10001, 10002, 10004
SLOPE = 0.01


def all_grads(A, c):
    return [c.grads_get(k) for k in A.PARAM_GROUPS]


def entries(T, mask=None):
    return int(LR.contributes(T, mask).sum())


def head_rows_input(pkg, ctx, ci):
    """The head's own input rows, tapped: the pooled rows on a readout context, else the last layer's output."""
    A = pkg.abi
    L = ci["cfg"].L - 1
    return ctx.tap(A.TAP_POOLED, L) if ci["readout"] is not None else ctx.tap(A.TAP_HOUT, L)


def check_count(pkg, ctx, ci, correct, mask):
    """BCE: n_correct within [sure, sure + |undecided|] of the head reference on the tapped rows; MSE: 0."""
    A = pkg.abi
    if ci["mode"] == LR.MSE:
        assert correct == 0
        return
    ref = LR.head_ref(head_rows_input(pkg, ctx, ci), ctx.params_get(A.PARAM_WO), ci["T"], mask, ci["mode"])
    sure, slack = LR.count_bounds(ref)
    parity.record("n_correct - sure", correct - sure, slack)
    assert sure <= correct <= sure + slack, (correct, sure, slack)


def compare_step(pkg, ctx, ci, ref, loss, tol):
    """loss / contributing entries, GAT_TAP_Y, hout of every layer, every parameter-group gradient."""
    A = pkg.abi
    n = max(1, entries(ci["T"], ci["mask"]))
    FC.compare(pkg, ctx, dict(ci["g"], n=n), ci["cfg"], ref, loss, tol, ["hout"], FC.GROUPS[:7])
    parity.check_abs("y", ctx.tap(A.TAP_Y), ref["y"], tol)
    got = ctx.grads_get(A.PARAM_WE)
    if ref.get("We") is None:
        assert got.size == 0
    else:
        parity.check_rel("grad We", got, ref["We"].grad.numpy(), tol)


# -- 1. the whole step against the fp64 model
STEP_CASES = LR.step_cases(FC)


@pytest.mark.parametrize("case", STEP_CASES, ids=[LR.case_id(c) for c in STEP_CASES])
def test_step_against_fp64(pkg, orc, case):
    A = pkg.abi
    ci = LR.step_inputs(case)
    ref = LR.model_of(ci)
    tol = 1e-2 if ci["bf16"] else TOL
    with LR.make_ctx(pkg, ci) as ctx:
        assert ctx.loss_info() == (A.LOSS_MODES[ci["mode"]], ci["g"]["c"])
        loss, correct = ctx.step()
        compare_step(pkg, ctx, ci, ref, loss, tol)
        check_count(pkg, ctx, ci, correct, ci["mask"])
        assert ctx.target_count() == entries(ci["T"], ci["mask"])
        if ci["mask"] is not None:                                       # the complement: gat_eval_mask and gat_target_count
            rest = ~ci["mask"]
            assert ctx.target_count(rest) == entries(ci["T"], rest) and ctx.target_count(ci["mask"]) == entries(ci["T"], ci["mask"])
            el, ec, en = ctx.eval_mask(rest)
            want = LR.head_ref(head_rows_input(pkg, ctx, ci), ctx.params_get(A.PARAM_WO), ci["T"], rest, ci["mode"])
            assert en == int(rest.sum())
            err = abs(el - want.l.sum()) / max(1, entries(ci["T"], rest))
            parity.record("eval loss/entries", err, TOL)
            assert err <= TOL
            sure, slack = LR.count_bounds(want)
            assert sure <= ec <= sure + slack


# -- 2. the head alone, on its own tapped inputs
HEAD_C = (1, 2, 3, 64, 65, 121, 128)
HEAD_LAST = ((8, 1), (8, 4), (4, 5), (8, 8), (4, 16), (2, 32))
HEAD_ROWS = (1, 127, 128, 129, 300)
HEAD_CASES = [(C, last, mode) for C in HEAD_C for last in HEAD_LAST for mode in LR.MODES]


def run_head_case(pkg, C, last, n, mode, how, T=None, wo_scale=1.0, masked=None):
    """One small one-layer context in `mode`, one step (how = "step") or forward + backward; every output of the head against
    loss_ref.head_ref on the tapped H_L.  -> (ctx outputs, reference) for the callers that look further."""
    A = pkg.abi
    H, DL = last
    case = HC.Case(f"loss-{mode}-C{C}-h{H}d{DL}-n{n}", C, last, n=n, layers=1, in_dim=10)
    inp = HC.make_inputs(case)
    masked = (n in (129, 300)) if masked is None else masked
    mask = LR.row_mask(n, seed=n) if masked and n > 2 else None
    if T is None:
        T = LR.targets_for(pkg, mode, n, C, seed=C * 1000 + n)
    Wo = (inp["Wo"] * np.float32(wo_scale)).astype(np.float32)
    refused = C * DL > 2048
    with pkg.GatContext(case.heads, case.outdims, case.in_dim, C) as ctx:
        ctx.set_loss(mode)
        ctx.set_graph(inp["rp"], inp["ci"]); ctx.set_features(inp["x"]); ctx.set_targets(T)
        ctx.params_set(A.PARAM_W, inp["W"]); ctx.params_set(A.PARAM_A, inp["a"]); ctx.params_set(A.PARAM_WO, Wo)
        if mask is not None:
            ctx.set_train_mask(mask)
        ctx.zero_grad()
        if refused:
            HC._expect_refusal(A, ctx.step if how == "step" else (lambda: (ctx.forward(), ctx.backward())))
            loss, correct = ctx.forward()                                # the context is still usable after the refusal
        elif how == "step":
            loss, correct = ctx.step()
        else:
            loss, correct = ctx.forward()
            ctx.backward()
        HL, hpre = ctx.tap(A.TAP_HOUT, 0), ctx.tap(A.TAP_HPRE, 0)
        y = ctx.tap(A.TAP_Y)
        gWo = g = None
        if not refused:
            gWo = ctx.grads_get(A.PARAM_WO).reshape(C, DL)
            g = ctx.tap(A.TAP_G, 0)
    ref = LR.head_ref(HL, Wo, T, mask, mode)
    return dict(loss=loss, correct=correct, y=y, gWo=gWo, g=g, HL=HL, hpre=hpre, mask=mask, T=T, refused=refused, H=H, DL=DL), ref


def run_wo(C, last, n, wo_scale):
    """The Wo [C][D_last] run_head_case uses for the BCE case of this shape (fp64 copy of the fp32 values)."""
    case = HC.Case(f"loss-{LR.BCE}-C{C}-h{last[0]}d{last[1]}-n{n}", C, last, n=n, layers=1, in_dim=10)
    return (HC.make_inputs(case)["Wo"] * np.float32(wo_scale)).astype(np.float32).astype(np.float64)


def check_head(out, ref, mode, B_loss=0.0, B_y=0.0):
    n_on = max(1, int(ref.on.sum()))
    assert np.isfinite(out["y"]).all() and np.isfinite(out["loss"])
    err = np.abs(out["y"].astype(np.float64) - ref.y).max()
    parity.record("y", err, TOL + B_y)
    assert err <= TOL + B_y, (err, TOL, B_y)
    err = abs(out["loss"] - ref.l.sum()) / n_on
    parity.record("loss/entries", err, TOL + B_loss)
    assert err <= TOL + B_loss, (err, TOL, B_loss)
    if mode == LR.MSE:
        assert out["correct"] == 0
    else:
        sure, slack = LR.count_bounds(ref)
        assert sure <= out["correct"] <= sure + slack, (out["correct"], sure, slack)
    if out["refused"]:
        return
    hp = out["hpre"].astype(np.float64).reshape(-1, out["H"], out["DL"])
    want_g = ref.gH[:, None, :] * np.where(hp > 0, 1.0, SLOPE) / out["H"]
    if B_y == 0.0:
        if np.abs(ref.gradWo).max() > 0:
            parity.check_rel("gradWo", out["gWo"], ref.gradWo)
        else:
            assert not out["gWo"].any()
        if np.abs(want_g).max() > 0:
            parity.check_rel("g", out["g"].reshape(want_g.shape), want_g)
        else:
            assert not out["g"].any()
    if out["mask"] is not None:
        assert not out["g"].reshape(want_g.shape)[~out["mask"]].any()    # dz is exactly 0 outside the training mask


@pytest.mark.parametrize("C,last,mode", HEAD_CASES, ids=[f"C{c}-h{l[0]}d{l[1]}-{m}" for c, l, m in HEAD_CASES])
def test_head_alone(pkg, C, last, mode):
    for n in HEAD_ROWS:
        for how in ("step", "fwdbwd"):
            out, ref = run_head_case(pkg, C, last, n, mode, how)
            check_head(out, ref, mode)


# -- 3. missing entries
@pytest.mark.parametrize("mode", LR.MODES)
@pytest.mark.parametrize("how", ["step", "fwdbwd"])
def test_missing_entries(pkg, mode, how):
    C, last, n = 5, (8, 8), 200
    base = LR.targets_for(pkg, mode, n, C, seed=77)
    T = base.copy(); T[17, :] = np.nan; T[:, 3] = np.nan                 # a whole row and a whole column
    out, ref = run_head_case(pkg, C, last, n, mode, how, T=T, masked=False)
    check_head(out, ref, mode)
    assert not out["gWo"][3].any()                                       # the column's dz is exactly 0
    assert not out["g"].reshape(n, -1)[17].any()                         # the row's gH is exactly 0
    out, ref = run_head_case(pkg, C, last, n, mode, how, T=np.full((n, C), np.nan, np.float32), masked=False)
    assert out["loss"] == 0.0 and out["correct"] == 0
    assert not out["gWo"].any() and not out["g"].any()
    assert np.isfinite(out["y"]).all()


def test_all_missing_whole_model(pkg, orc):
    """All entries NaN through the whole step: loss 0, every gradient of every group exactly 0, no NaN anywhere."""
    A = pkg.abi
    ci = LR.step_inputs(("records_d8", "plain", LR.BCE))
    with LR.make_ctx(pkg, ci, T=np.full_like(ci["T"], np.nan)) as ctx:
        assert ctx.step() == (0.0, 0)
        for k, gk in enumerate(all_grads(A, ctx)):
            assert not gk.any() and np.isfinite(gk).all(), k
        assert ctx.target_count() == 0


# -- 4. saturation
@pytest.mark.parametrize("how", ["step", "fwdbwd"])
def test_bce_saturated(pkg, how):
    """Wo x 50: |z| of the order 10^2.  Loss, y and gradients stay finite and within TOL + B of the reference, B the fp32 rounding
    bound of the logits (the loss has |dl/dz| <= 1, the sigmoid 1/4; gradWo[c][d] moves by at most sum_r B[r][c] |X[r][d]| / 4)."""
    C, last, n = 7, (8, 8), 200
    out, ref = run_head_case(pkg, C, last, n, LR.BCE, how, wo_scale=50.0, masked=False)
    assert 50.0 <= np.abs(ref.z).max(), np.abs(ref.z).max()
    check_head(out, ref, LR.BCE, B_loss=float(ref.bound[ref.on].mean()), B_y=float(ref.bound.max()))
    assert np.isfinite(out["gWo"]).all() and np.isfinite(out["g"]).all()
    slack = (np.where(ref.on, ref.bound, 0.0) / 4).T @ np.abs(out["HL"].astype(np.float64))
    err = np.abs(out["gWo"] - ref.gradWo)
    assert np.all(err <= GTOL * np.abs(ref.gradWo).max() + slack), float((err - slack).max())
    Wo64 = np.abs(run_wo(C, last, n, 50.0))
    slack_g = ((np.where(ref.on, ref.bound, 0.0) / 4) @ Wo64)[:, None, :] / last[0]       # gH moves by sum_c B[r][c] |Wo[c][d]| / 4
    hp = out["hpre"].astype(np.float64).reshape(n, last[0], last[1])
    want_g = ref.gH[:, None, :] * np.where(hp > 0, 1.0, SLOPE) / last[0]
    err = np.abs(out["g"].reshape(want_g.shape) - want_g)
    assert np.all(err <= GTOL * np.abs(want_g).max() + slack_g), float((err - slack_g).max())


# -- 5. bitwise identities
@pytest.mark.parametrize("mode", LR.MODES)
def test_paths_agree_bitwise(pkg, orc, mode):
    A = pkg.abi
    ci = LR.step_inputs(("records_d8", "plain", mode))
    with LR.make_ctx(pkg, ci) as s1, LR.make_ctx(pkg, ci) as fb, LR.make_ctx(pkg, ci) as ph, LR.make_ctx(pkg, ci) as gr:
        l1 = s1.step(); g1 = all_grads(A, s1)
        s1.zero_grad()
        assert s1.step() == l1                                           # two runs of one context
        for a, b in zip(all_grads(A, s1), g1):
            assert np.array_equal(a, b)
        lf = fb.forward(); fb.backward(); gf = all_grads(A, fb)
        for l in range(2):
            ph.layer_project(l); ph.layer_forward_edges(l)
        lp = ph.head_forward()
        ph.head_backward()
        for l in (1, 0):
            ph.layer_backward_edges(l); ph.layer_backward_dense(l)
        gp = all_grads(A, ph)
        assert lf == l1 and lp == l1
        for k in A.PARAM_GROUPS:
            assert np.array_equal(gf[k], g1[k]) and np.array_equal(gp[k], g1[k]), k
        gr.step_graph(True)
        for _ in range(3):                                               # eager warm-up, capture + replay, replay
            gr.zero_grad()
            assert gr.step() == l1
            for k in A.PARAM_GROUPS:
                assert np.array_equal(gr.grads_get(k), g1[k]), k
        # new targets between two replays: the captured step reads them through the same buffer
        T2 = LR.targets_for(pkg, mode, ci["g"]["n"], ci["g"]["c"], seed=123)
        gr.set_targets(T2)
        gr.zero_grad()
        l2 = gr.step()
        with LR.make_ctx(pkg, ci, T=T2) as fresh:
            assert fresh.step() == l2 and l2 != l1
            for k in A.PARAM_GROUPS:
                assert np.array_equal(gr.grads_get(k), fresh.grads_get(k)), k


# -- 6. mode 0 is the parent
def test_mode0_is_the_parent(pkg, orc):
    A = pkg.abi
    g = FC.parity_graph()
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    P = orc.xavier_params(cfg, 3)
    outs = []
    for call in (False, True):
        with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"], collect_timing=True) as c:
            if call:
                c.set_loss(0)
            c.set_graph(g["row_ptr"], g["col_idx"]); c.set_features(g["x"]); c.set_labels(g["labels"])
            for grp, arr in enumerate(P):
                c.params_set(grp, arr)
            c.zero_grad()
            c.kernel_stats_reset()
            res = c.step()
            outs.append((res, all_grads(A, c), {k: v[0] for k, v in c.kernel_stats().items()}, c.algorithmic_bytes()))
            assert c.loss_info() == (0, g["c"])
    (ra, ga, sa, ba), (rb, gb, sb, bb) = outs
    assert ra == rb and sa == sb and ba == bb
    for a, b in zip(ga, gb):
        assert np.array_equal(a, b)
    ci = LR.step_inputs(("records_d8", "plain", LR.BCE))                 # on: the documented byte terms
    with LR.make_ctx(pkg, ci) as r:
        _, pr = r.algorithmic_bytes()
        N, Cn = g["n"], g["c"]
        for k in ("head_forward", "head_backward"):
            assert pr[k] - ba[1][k] == 4.0 * N * (Cn - 1)
        assert all(pr[k] == ba[1][k] for k in pr if k not in ("head_forward", "head_backward"))


# -- 7. readout
@pytest.mark.parametrize("case", LR.READOUT_CASES, ids=[LR.case_id(c) for c in LR.READOUT_CASES])
def test_readout_against_fp64(pkg, orc, case):
    A = pkg.abi
    ci = LR.readout_inputs(case)
    ref = LR.model_of(ci)
    with LR.make_ctx(pkg, ci) as ctx:
        loss, correct = ctx.step()
        compare_step(pkg, ctx, ci, ref, loss, TOL)
        check_count(pkg, ctx, ci, correct, ci["mask"])
        G = len(ci["graph_ptr"]) - 1
        assert ctx.tap(A.TAP_Y).shape == (G, ci["g"]["c"])
        assert ctx.target_count() == entries(ci["T"], ci["mask"])
        with pytest.raises(A.GatError) as ei:
            ctx.set_targets(np.zeros((ci["g"]["n"], ci["g"]["c"]), np.float32))        # per node: the wrong row count
        assert ei.value.code == E_INVALID


# -- 8. optimizers
def test_optimizers_on_mse_gradients(pkg, orc):
    """One Adam step and one clipped SGD step on the gradients of an MSE step, against fp64 arithmetic on those same gradients.  Bars: the
    update is fp32 arithmetic on O(1) operands — GTOL of the largest update of the group (the clip's norm is an fp32 sum of a few
    thousand squares) plus one ulp (2^-23) of the parameter."""
    A = pkg.abi
    ci = LR.step_inputs(("records_d8", "plain", LR.MSE))
    lr, b1, b2, eps, thresh = 0.01, 0.9, 0.999, 1e-8, 0.5
    groups = (A.PARAM_W, A.PARAM_A, A.PARAM_WO)
    for opt in ("adam", "sgd_clip"):
        with LR.make_ctx(pkg, ci) as ctx:
            ctx.step()
            before, want = {}, {}
            for k in groups:
                p0, gk = ctx.params_get(k).astype(np.float64), ctx.grads_get(k).astype(np.float64)
                w = p0.copy()
                if opt == "adam":
                    FC.adam64(w, gk, np.zeros_like(gk), np.zeros_like(gk), lr, b1, b2, eps, 1)
                else:
                    norm = np.sqrt((gk * gk).sum())
                    assert norm > thresh                                 # the clip is active
                    w -= lr * gk * (thresh / (norm + 1e-9))
                before[k], want[k] = p0, w
            if opt == "adam":
                ctx.step_adam(lr, b1, b2, eps, 1)
            else:
                ctx.clip(thresh)
                ctx.step_sgd(lr)
            for k in groups:
                step = np.abs(want[k] - before[k]).max()
                assert step > 0
                bar = GTOL * step + 2.0 ** -23 * np.abs(want[k])
                err = np.abs(ctx.params_get(k).astype(np.float64) - want[k])
                parity.record(f"{opt} group {k}", float((err / bar).max()), 1.0)
                assert np.all(err <= bar), (opt, k, float((err - bar).max()))


# -- 9. shards
def test_two_shards_on_the_host_transport(pkg, orc):
    """Two processes sharing the GPU, BCE with missing entries: loss, count and gradients equal the one-GPU result at shard_cases.XTOL."""
    A = pkg.abi
    g, P, T = LR.shard_setup(pkg, orc)
    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as one:
        one.set_loss("bce")
        one.set_graph(g["row_ptr"], g["col_idx"]); one.set_features(g["x"]); one.set_targets(T)
        for grp, arr in enumerate(P):
            one.params_set(grp, arr)
        one.zero_grad()
        loss1, correct1 = one.step()
        want = np.concatenate([one.grads_get(k) for k in range(3)])
    world = 2
    with tempfile.TemporaryDirectory() as d:
        shm = f"/gatv2_loss_{os.getpid()}"
        code = ("import sys; sys.path.insert(0, {t!r}); import loss_ref; loss_ref.shard_worker({r}, {w}, {d!r}, {s!r})")
        kids = [subprocess.Popen([sys.executable, "-c", code.format(t=os.path.join(ROOT, "tests"), r=r, w=world, d=d, s=shm)],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
        failed = None
        for r, k in enumerate(kids):                                     # each child under its own limit; nothing more starts after a failure
            try:
                out, _ = k.communicate(timeout=120)
            except subprocess.TimeoutExpired:
                failed = (r, "timeout")
                break
            if k.returncode != 0:
                failed = (r, out)
                break
        if failed is not None:
            for k in kids:
                if k.poll() is None:
                    k.kill()
                    k.communicate()
            raise AssertionError(f"rank {failed[0]} failed: {failed[1]}")
        outs = [np.load(os.path.join(d, f"r{r}.npz")) for r in range(world)]
    X = shard_cases.XTOL
    for o in outs:
        assert abs(float(o["loss"]) - loss1) <= X * max(1.0, abs(loss1)) and int(o["correct"]) == correct1
        parity.record("grads", parity.rel_err(o["grads"], want), X)
        assert np.abs(o["grads"] - want).max() <= X * np.abs(want).max()
        assert np.array_equal(o["grads"], outs[0]["grads"])


# -- 10. state and argument rules
def test_state_and_argument_rules(pkg, orc):
    import torch
    A = pkg.abi
    dev = torch.device("cuda:0")
    g = FC.parity_graph()
    n, C = g["n"], g["c"]
    T = LR.targets_for(pkg, LR.BCE, n, C)

    def refused(code, fn, text=None):
        with pytest.raises(A.GatError) as ei:
            fn()
        assert ei.value.code == code, str(ei.value)
        if text is not None:
            assert text in str(ei.value), str(ei.value)

    def fresh(mode=None, **kw):
        c = pkg.GatContext([8, 8], [8, 8], g["f"], C, **kw)
        if mode is not None:
            c.set_loss(mode)
        c.set_graph(g["row_ptr"], g["col_idx"]); c.set_features(g["x"])
        return c

    with fresh() as c:                                                   # mode 0
        refused(E_INVALID, lambda: c.set_loss(3))
        refused(E_INVALID, lambda: c.set_loss(-1))
        refused(E_STATE, lambda: c.set_targets(T))                       # softmax takes labels
        c.set_loss("softmax")
        c.set_labels(g["labels"])
        refused(E_STATE, lambda: c.set_loss("bce"))                      # after the labels
        refused(E_STATE, lambda: c.set_loss(0))
        refused(E_STATE, lambda: c.target_count())
    with pkg.GatContext([8, 8], [8, 8], g["f"], C) as c:                 # before the graph
        c.set_loss("mse")
        refused(E_STATE, lambda: c.set_targets(T))
    with fresh("bce") as c:
        assert c.loss_info() == (A.LOSS_BCE, C)
        refused(E_STATE, lambda: c.set_labels(g["labels"]), "gat_set_targets")
        d_lab = torch.from_numpy(g["labels"]).to(dev)
        refused(E_STATE, lambda: c.set_labels_device(d_lab.data_ptr(), n), "gat_set_targets")
        c.params_init(1)
        refused(E_STATE, lambda: c.step(), "targets")                    # a step without targets says so
        refused(E_STATE, lambda: c.head_forward(), "targets")
        refused(E_INVALID, lambda: c.set_targets(T[:, :C - 1]))
        refused(E_INVALID, lambda: c.set_targets(T[:n - 1]))
        refused(E_UNSUPPORTED, lambda: c.set_targets_device(d_lab.data_ptr(), (1 << 31) // C + 1, C))      # n_rows * C >= 2^31
        for bad_v, idx in ((1.5, 7), (-0.25, 3 * C + 1), (np.inf, 11), (-np.inf, 5)):
            bad = np.nan_to_num(T, nan=0.5).astype(np.float32)
            bad[-1, -1] = 2.0                                            # a later offender: the LOWEST index is reported
            bad.reshape(-1)[idx] = bad_v
            refused(E_INVALID, lambda: c.set_targets(bad), f"entry {idx} ")
            d_bad = torch.from_numpy(bad).to(dev)
            refused(E_INVALID, lambda: c.set_targets_device(d_bad.data_ptr(), n, C), f"entry {idx} ")
        refused(E_STATE, lambda: c.step(), "targets")                    # nothing stuck
        d_T = torch.from_numpy(T).to(dev)
        c.set_targets_device(d_T.data_ptr(), n, C)                       # the device form, NaN entries included
        refused(E_STATE, lambda: c.set_loss("mse"))                      # after the targets
        c.zero_grad()
        res = c.step()
        with LR.make_ctx(pkg, dict(LR.step_inputs(("records_d8", "plain", LR.BCE)), P=[c.params_get(k) for k in range(3)])) as h:
            assert h.step() == res                                       # the host form gives the same
        refused(E_INVALID, lambda: c.set_train_mask(np.ones(n + 1, bool)))
        refused(E_INVALID, lambda: c.target_count(np.ones(n + 1, bool)))
    with fresh("mse") as c:
        ok = np.nan_to_num(LR.targets_for(pkg, LR.MSE, n, C), nan=0.0).astype(np.float32)
        ok[0, 0] = -7.5                                                  # MSE targets are any finite value
        c.set_targets(ok)
        bad = ok.copy(); bad.reshape(-1)[9] = np.inf
        refused(E_INVALID, lambda: c.set_targets(bad), "entry 9 ")
        refused(E_INVALID, lambda: c.set_targets(ok[:, :2]))             # a later call keeps the shape
    with pkg.GatContext([8, 8], [8, 8], g["f"], C, flat_lrelu_index=True) as c:
        refused(E_UNSUPPORTED, lambda: c.set_loss("bce"), "flat_lrelu_index")
        c.set_loss(0)                                                    # mode 0 is always accepted before the labels


SWITCH_SNIPPET = """
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as entry
import loss_ref as LR
pkg = entry.load_package(); A = pkg.abi
ci = LR.step_inputs(("records_d8", "plain", {mode!r}))
try:
    with LR.make_ctx(pkg, ci) as ctx:
        loss = ctx.step()
        np.save({out!r}, np.concatenate([ctx.grads_get(k) for k in A.PARAM_GROUPS]))
        print("LOSS", repr(loss[0]), loss[1], "|", A.switches())
except A.GatError as e:
    print("CODE", e.code, "|", str(e)[:120])
"""


def test_experiment_library_and_form_switch(pkg, orc, tmp_path):
    """Switches are read once per process, so each setting is a process of its own (two at a time).  The experiment library with
    GAT_DBG set refuses gat_set_loss(BCE / MSE) with GAT_E_UNSUPPORTED and a text naming the call.  GAT_LOSS_BLOCKED=0 forces the
    any-shape form of the head kernels at a shape the register-blocked form would take (C = 5, D_last = 8): the same loss terms and
    products in another order of summation — loss and every gradient within 1e-5 of the default's, the count equal."""
    from conftest import run_snippets_parallel
    exp = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "libgatv2_hip_exp.so")
    assert os.path.exists(exp)
    jobs = {}
    for mode in LR.MODES:
        for key, env in (("default", {}), ("any_shape", {"GAT_LOSS_BLOCKED": "0"}), ("experiment", {"GATV2_LIB": exp, "GAT_DBG": "1"})):
            jobs[(mode, key)] = (SWITCH_SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), mode=mode,
                                                       out=str(tmp_path / f"{mode}_{key}.npy")), env)
    res = run_snippets_parallel(jobs, workers=2, timeout=120)
    for key, r in res.items():
        assert r.returncode == 0, (key, r.stderr[-2000:])
    for mode in LR.MODES:
        out = res[(mode, "experiment")].stdout
        assert "CODE 10004" in out and "gat_set_loss" in out, out
        d, a = res[(mode, "default")].stdout.split(), res[(mode, "any_shape")].stdout.split()
        assert d[0] == a[0] == "LOSS" and "GAT_LOSS_BLOCKED=0" in res[(mode, "any_shape")].stdout
        assert "GAT_LOSS_BLOCKED" not in res[(mode, "default")].stdout
        assert abs(float(d[1]) - float(a[1])) <= 1e-5 * abs(float(d[1])) and d[2] == a[2]
        gd, ga = np.load(tmp_path / f"{mode}_default.npy"), np.load(tmp_path / f"{mode}_any_shape.npy")
        assert np.abs(gd).max() > 0 and np.abs(gd - ga).max() <= 1e-5 * np.abs(gd).max()


# -- 11. the host program
def write_dataset(d, g, T, gp=None):
    os.makedirs(d)
    np.savetxt(os.path.join(d, "row_ptr.txt"), g["row_ptr"], fmt="%d")
    np.savetxt(os.path.join(d, "col_idx.txt"), g["col_idx"], fmt="%d")
    np.savetxt(os.path.join(d, "features.txt"), g["x"], fmt="%.9g")
    np.savetxt(os.path.join(d, "targets.txt"), T, fmt="%.9g")
    if gp is not None:
        np.savetxt(os.path.join(d, "graph_ptr.txt"), gp, fmt="%d")


@pytest.mark.parametrize("mode,readout", [("mse", "mean"), ("bce", None)])
def test_train_edge_loss(pkg, orc, mode, readout):
    """train_edge --loss on a dataset folder written here: three epochs match a GatContext driven the same way."""
    assert os.path.exists(BIN), "build() makes the host binary"
    g = FC.host_graph(3)
    gp = np.array([0, 7, 7, 20, 40], np.int32) if readout else None
    rows = len(gp) - 1 if readout else g["n"]
    C = 3
    T = LR.targets_for(pkg, mode, rows, C, seed=21)
    with tempfile.TemporaryDirectory() as root:
        d = os.path.join(root, "tiny")
        write_dataset(d, g, T, gp)
        x = np.loadtxt(os.path.join(d, "features.txt"), dtype=np.float32, ndmin=2)      # exactly what the binary reads
        Tt = np.loadtxt(os.path.join(d, "targets.txt"), dtype=np.float32, ndmin=2)
        env = dict(os.environ)
        env.pop("DATA_ROOT", None)
        args = [BIN, "--dataset", "tiny", "--data-root", root, "--epochs", "3", "--optimizer", "adam", "--lr", "0.01", "--clip",
                "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8", "--seed", "7", "--loss", mode]
        r = subprocess.run(args + (["--readout", readout] if readout else []), capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = re.findall(r"Avg Loss: ([0-9.]+)(?:, Accuracy: ([0-9.]+)%)?", r.stdout)
        assert len(got) == 3, r.stdout
    n_on = entries(Tt)
    with pkg.GatContext([8, 8], [8, 8], g["f"], C) as ctx:
        ctx.set_loss(mode)
        ctx.set_graph(g["row_ptr"], g["col_idx"]); ctx.set_features(x)
        if readout:
            ctx.set_readout(readout, graph_ptr=gp)
        ctx.set_targets(Tt)
        assert ctx.target_count() == n_on
        ctx.params_init(7)
        ctx.zero_grad()
        for t, (loss_txt, acc_txt) in enumerate(got, 1):                 # the host's epoch: forward, backward, clip, adam, zero_grad
            loss, correct = ctx.forward()
            ctx.backward()
            ctx.clip(5.0)
            ctx.step_adam(0.01, 0.9, 0.999, 1e-8, t)
            ctx.zero_grad()
            assert loss_txt == "%f" % (np.float32(loss) / n_on), (t, loss_txt, loss / n_on)
            if mode == "bce":
                assert acc_txt == "%.2f" % (100.0 * np.float32(np.float32(correct) / n_on)), (t, acc_txt, correct)
            else:
                assert acc_txt == ""
