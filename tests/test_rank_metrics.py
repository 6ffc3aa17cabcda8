"""Ranking metrics on the GPU (include/gatv2_abi.h "ranking metrics"): gat_op_rank_stats against the numpy law of tests/rank_ref.py on
every case of tests/rank_cases.py — integers exactly, ap and mrr within (n_pos + 2) * 2^-52 relative, two calls bitwise equal, the padded
score rows untouched; gat_eval_rank on four contexts (a pair head with BCE and sampled negatives, a softmax node head, a BCE node head with
NaN targets, a readout) against the law applied to tap(GAT_TAP_Y), after a forward and after a fused step, with the steps after the call
bitwise those of a run without it, also across a captured replay, whose state the call leaves as it found it and whose rankings are
bitwise the eager run's; the refusal matrix; the train_edge host.

tests/test_rank_metrics_cpu.py proves on the host that the reference is the pairwise law and sklearn's, and asserts the conditions of
the generated cases (both classes per column, the tie groups, the saturated column)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import feature_cases as FC
import rank_cases as RC
import rank_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
E_INVALID, E_STATE, E_UNSUPPORTED = 10001, 10002, 10004


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the seam tests need the GPU"
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def seam_refs():
    """rank_ref on every seam case with the eight K, computed once and shared."""
    return {c["name"]: RR.rank_stats(c["scores"], c["labels"], c["targets"], c["mask"], ks=RC.KS8) for c in RC.seam_cases()}


def bitwise(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint64) if a[k].dtype == np.float64 else a[k],
                              np.asarray(b[k]).view(np.uint64) if b[k].dtype == np.float64 else b[k]) for k in ("ap", "mrr", *RR.INT_KEYS))


# -- the seam
@pytest.mark.parametrize("case", RC.seam_cases(), ids=RC.seam_ids())
def test_seam_is_the_law(pkg, torch_dev, seam_refs, case):
    torch, dev = torch_dev
    A = pkg.abi
    host = RC.padded(case)
    d_s = torch.from_numpy(host).to(dev)
    keep = [d_s]
    kw = {}
    for name, arr, dt in (("d_labels", case["labels"], np.int32), ("d_targets", case["targets"], np.float32), ("d_mask", case["mask"], np.uint8)):
        if arr is not None:
            keep.append(torch.from_numpy(np.ascontiguousarray(arr, dt)).to(dev))
            kw[name] = keep[-1].data_ptr()

    def call(ks):
        return A.op_rank_stats(d_s.data_ptr(), case["stride"], case["rows"], case["cols"], ks=ks, **kw)

    want8 = seam_refs[case["name"]]
    got8 = call(RC.KS8)
    RR.assert_same(got8, want8, (case["name"], "8 K"))
    assert np.array_equal(got8["auc"], want8["auc"], equal_nan=True) and np.array_equal(got8["hits_at"], want8["hits_at"], equal_nan=True)
    assert bitwise(got8, call(RC.KS8)), "two calls differ"
    ks = RC.case_ks(case, int(want8["n_neg"][0]))
    RR.assert_same(call(ks), RR.rank_stats(case["scores"], case["labels"], case["targets"], case["mask"], ks=ks), (case["name"], ks))
    none = call(())
    assert none["hits"].shape == (case["cols"], 0)
    RR.assert_same(dict(none, hits=want8["hits"][:, :0]), dict(want8, hits=want8["hits"][:, :0]), (case["name"], "no K"))
    if case["law"] == "equal":
        assert np.array_equal(got8["auc_num"].astype(np.int64), got8["n_pos"] * got8["n_neg"])
    back = d_s.cpu().numpy()
    assert np.array_equal(back.view(np.uint32), host.view(np.uint32)), "the score rows or the floats behind them changed"


# -- the contexts
def supervision(cc):
    return dict(labels=cc["labels"], targets=cc["targets"], mask=cc["mask"])


@pytest.mark.parametrize("name", RC.CONTEXTS)
def test_context_is_the_law_on_the_y_tap(pkg, name):
    A = pkg.abi
    cc = RC.context_case(name)
    with RC.make_context(pkg, cc) as ctx:
        ctx.forward()
        y = ctx.tap(A.TAP_Y).reshape(cc["rows"], cc["C"])
        want = RR.rank_stats(y, ks=RC.CTX_KS, **supervision(cc))
        assert ((want["n_pos"] > 0) & (want["n_neg"] > 0)).sum() >= max(cc["C"] - 1, 1) and want["n_nan"].sum() == 0
        got = ctx.eval_rank(cc["mask"], RC.CTX_KS)
        RR.assert_same(got, want, (name, "after forward"))
        assert np.array_equal(got["auc"], want["auc"], equal_nan=True)
        assert bitwise(got, ctx.eval_rank(cc["mask"], RC.CTX_KS))
        other = ~cc["mask"]                              # another split of the same forward
        RR.assert_same(ctx.eval_rank(other, (2,)), RR.rank_stats(y, ks=(2,), **dict(supervision(cc), mask=other)), (name, "other mask"))
        ctx.zero_grad()
        ctx.step()                                       # the fused head step leaves y invalid: the call re-runs the head's forward
        got2 = ctx.eval_rank(cc["mask"], RC.CTX_KS)
        y2 = ctx.tap(A.TAP_Y).reshape(cc["rows"], cc["C"])
        RR.assert_same(got2, RR.rank_stats(y2, ks=RC.CTX_KS, **supervision(cc)), (name, "after step"))
        assert np.array_equal(y2, y) and bitwise(got2, got)      # no optimizer ran: the same forward, the same answer


def run_steps(pkg, cc, n_steps, rank_before=(), graph=False):
    """n_steps gat_step on a fresh context with an Adam update between them; rank_before: the steps in front of which eval_rank is called.
    -> per step (loss, correct, every gradient group), the eval_rank results in call order, the replay state seen around each call."""
    A = pkg.abi
    out, ranks, states = [], [], []
    with RC.make_context(pkg, cc) as ctx:
        if graph:
            ctx.step_graph(True)
        for i in range(n_steps):
            if i in rank_before:
                before = ctx.step_graph_state()
                ranks.append(ctx.eval_rank(cc["mask"], RC.CTX_KS))
                states.append((before, ctx.step_graph_state()))
            res = ctx.step()
            out.append((res, [ctx.grads_get(k) for k in A.PARAM_GROUPS]))
            ctx.step_adam(0.01, 0.9, 0.999, 1e-8, i + 1)
            ctx.zero_grad()
        ranks.append(ctx.eval_rank(cc["mask"], RC.CTX_KS))               # of the last step's forward
    return out, ranks, states


def same_steps(a, b, what):
    for i, ((res_a, g_a), (res_b, g_b)) in enumerate(zip(a, b)):
        assert res_a == res_b, (what, i, res_a, res_b)
        for k, (x, y) in enumerate(zip(g_a, g_b)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, i, k)


@pytest.mark.parametrize("name", RC.CONTEXTS)
def test_steps_after_the_call_are_bitwise_unchanged(pkg, name):
    """eval_rank in front of steps 1 .. 4 and behind the last, eagerly and under gat_step_graph (after the warm-up, after the capture and
    between replays).  Every step is bitwise the step of a run without the call; the replay state the call finds is the state it leaves
    (armed after the warm-up, captured from then on: not re-armed); and every ranking under replay is bitwise the eager run's at the
    same point — the steps are the same, so a replayed run that ranked the y of an earlier evaluation would differ."""
    cc = RC.context_case(name)
    before = (1, 2, 3, 4)
    plain, _, _ = run_steps(pkg, cc, 5)
    eager, eager_ranks, eager_states = run_steps(pkg, cc, 5, rank_before=before)
    plain_g, _, _ = run_steps(pkg, cc, 5, graph=True)
    replay, replay_ranks, replay_states = run_steps(pkg, cc, 5, rank_before=before, graph=True)
    same_steps(plain, eager, (name, "eager"))
    same_steps(plain_g, replay, (name, "replay"))
    same_steps(plain, replay, (name, "replay against eager"))
    assert eager_states == [(0, 0)] * 4 and replay_states == [(1, 1), (2, 2), (2, 2), (2, 2)], (eager_states, replay_states)
    assert len(eager_ranks) == len(replay_ranks) == 5
    for i, (a, b) in enumerate(zip(eager_ranks, replay_ranks)):
        assert bitwise(a, b), (name, "ranking", i)
    # the parameters move between the steps, so the rankings do: a stale y would have been seen
    moved = [not bitwise(eager_ranks[i], eager_ranks[i + 1]) for i in range(4)]
    print(name, "rankings that differ from the one before:", moved)
    assert all(moved), (name, moved)


# -- refusals
def refused(A, code, fn, text=None):
    with pytest.raises(A.GatError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    if text is not None:
        assert text in str(ei.value), str(ei.value)


def test_refusal_matrix(pkg):
    A = pkg.abi
    cc = RC.context_case("node_softmax")
    g, n = cc["g"], cc["rows"]
    mask = cc["mask"]
    with pkg.GatContext(RC.HEADS, RC.OUTDIMS, g["f"], g["c"]) as c:
        c.set_graph(g["row_ptr"], g["col_idx"]); c.set_features(g["x"])
        refused(A, E_STATE, lambda: c.eval_rank(mask))                           # before the labels
        c.set_labels(g["labels"]); c.params_init(1)
        refused(A, E_STATE, lambda: c.eval_rank(mask), "no forward yet")           # before any forward
        refused(A, E_INVALID, lambda: c.eval_rank(mask, range(1, 10)), "n_ks")
        refused(A, E_INVALID, lambda: c.eval_rank(mask, (5, 0)), "K must be >= 1")
        c.forward()
        refused(A, E_INVALID, lambda: c.eval_rank(mask[:-1]), "mask length")
        refused(A, E_INVALID, lambda: c.eval_rank(mask, range(1, 10)), "n_ks")
        refused(A, E_INVALID, lambda: c.eval_rank(mask, (5, -2)), "K must be >= 1")
        refused(A, E_INVALID, lambda: A._chk(c.lib.gat_eval_rank(c._ctx, None, n, None, 0, None)), "null")
        assert c.eval_rank(mask, range(1, 9))["hits"].shape == (g["c"], 8)       # and then it works, with all eight
    with pkg.GatContext(RC.HEADS, RC.OUTDIMS, g["f"], g["c"]) as c:                # MSE: no binary relevance
        c.set_loss("mse")
        c.set_graph(g["row_ptr"], g["col_idx"]); c.set_features(g["x"])
        c.set_targets(np.zeros((n, g["c"]), np.float32)); c.params_init(1)
        c.forward()
        refused(A, E_UNSUPPORTED, lambda: c.eval_rank(mask), "GAT_LOSS_MSE")
    S = pkg.shard                                        # a destination-range shard, without and with a transport
    plan = S.make_plan(g["row_ptr"], 2, 0)
    rp_l, ci_l = S.local_csr(plan, g["row_ptr"], g["col_idx"])
    with pkg.GatContext(RC.HEADS, RC.OUTDIMS, g["f"], g["c"]) as c:
        c.set_graph(rp_l, ci_l, n_table=plan.n_table, table_row0=plan.table_row0)
        c.set_source_features(plan.table_features(g["x"]))
        c.set_labels(g["labels"][plan.row0:plan.row0 + plan.n_rows]); c.params_init(1)
        m = mask[plan.row0:plan.row0 + plan.n_rows]
        refused(A, E_UNSUPPORTED, lambda: c.eval_rank(m), "shard")
    with pkg.GatContext(RC.HEADS, RC.OUTDIMS, g["f"], g["c"]) as c:                # world = 1 over the host transport: a transport all the same
        c.set_graph(g["row_ptr"], g["col_idx"]); c.set_features(g["x"]); c.set_labels(g["labels"]); c.params_init(1)
        c.comm_init_host(1, 0, "/gat_rank_refusal_%d" % os.getpid(), 4 * max(n * 64, c.n_params + 3))
        refused(A, E_UNSUPPORTED, lambda: c.eval_rank(mask), "transport")


# -- the host program
def run_host(root, extra, loss, epochs=3):
    env = dict(os.environ)
    env.pop("DATA_ROOT", None)
    r = subprocess.run([BIN, "--dataset", "tiny", "--data-root", root, "--epochs", str(epochs), "--optimizer", "adam", "--lr", "0.01", "--clip",
                        "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8", "--seed", "7", "--loss", loss, *extra],
                       capture_output=True, text=True, env=env, timeout=300)
    return r


def test_train_edge_rank_metrics(pkg):
    """--rank-metrics 1,10,50 prints, behind every validation line, the macro averages of rank_ref on the same forward; without the flag
    the program prints what it printed before the flag existed: the ranked run's output minus the new lines (times apart)."""
    assert os.path.exists(BIN), "build() makes the host binary"
    g = FC.host_graph(3)
    u, v, t = pkg.synth.link_pairs(g["row_ptr"], g["col_idx"], 60, 60, seed=2)
    P = len(u)
    val = np.random.default_rng(4).random(P) > 0.5
    ks = (1, 10, 50)
    with tempfile.TemporaryDirectory() as root:
        d = os.path.join(root, "tiny")
        os.makedirs(d)
        np.savetxt(os.path.join(d, "row_ptr.txt"), g["row_ptr"], fmt="%d")
        np.savetxt(os.path.join(d, "col_idx.txt"), g["col_idx"], fmt="%d")
        np.savetxt(os.path.join(d, "features.txt"), g["x"], fmt="%.9g")
        np.savetxt(os.path.join(d, "targets.txt"), t, fmt="%.9g")
        np.savetxt(os.path.join(d, "pairs.txt"), np.stack([u, v], 1), fmt="%d")
        np.savetxt(os.path.join(d, "val.txt"), val.astype(int), fmt="%d")
        np.savetxt(os.path.join(d, "train.txt"), (~val).astype(int), fmt="%d")
        x = np.loadtxt(os.path.join(d, "features.txt"), dtype=np.float32, ndmin=2)      # exactly what the binary reads
        common = ["--pairs", "mul", "--train-mask", os.path.join(d, "train.txt"), "--val-mask", os.path.join(d, "val.txt")]
        ranked = run_host(root, common + ["--rank-metrics", ",".join(map(str, ks))], "bce")
        plain = run_host(root, common, "bce")
        assert ranked.returncode == 0 and plain.returncode == 0, ranked.stdout + ranked.stderr + plain.stderr
        for extra, loss, text in ((["--pairs", "mul", "--rank-metrics", "1"], "bce", "needs --val-mask"),
                                  (common + ["--rank-metrics", "1"], "mse", "--loss mse"),
                                  (common + ["--rank-metrics", "1,0"], "bce", "K >= 1"),
                                  (common + ["--rank-metrics", "1,2,3,4,5,6,7,8,9"], "bce", "1 to 8"),
                                  (common + ["--rank-metrics", "3x"], "bce", "K >= 1"),
                                  (common + ["--rank-metrics", "1", "--ranks", "2"], "bce", "--ranks 1")):
            r = run_host(root, extra, loss)
            assert r.returncode != 0 and text in r.stderr, (extra, r.stderr)

    def lines(out):
        return [l for l in out.splitlines() if "total time" not in l and "GPU memory" not in l]
    rank_lines = [l for l in ranked.stdout.splitlines() if l.startswith("Val AUC:")]
    assert len(rank_lines) == 3
    assert [l for l in lines(ranked.stdout) if not l.startswith("Val AUC:")] == lines(plain.stdout)
    after = ranked.stdout.splitlines()
    for i, l in enumerate(after):
        if l.startswith("Val AUC:"):
            assert after[i - 1].startswith("Val Loss:")                 # one line after each validation line
    with pkg.GatContext([8, 8], [8, 8], g["f"], 1) as ctx:
        ctx.set_loss("bce")
        ctx.set_graph(g["row_ptr"], g["col_idx"]); ctx.set_features(x)
        ctx.set_pairs("mul", u, v)
        ctx.set_targets(t.reshape(P, 1))
        ctx.set_train_mask(~val)
        ctx.params_init(7)
        ctx.zero_grad()
        for e, line in enumerate(rank_lines, 1):
            ctx.forward()
            y = ctx.tap(pkg.abi.TAP_Y).reshape(P, 1)
            ctx.backward()
            ctx.clip(5.0)
            ctx.step_adam(0.01, 0.9, 0.999, 1e-8, e)
            ctx.zero_grad()
            st = RR.rank_stats(y, targets=t.reshape(P, 1), mask=val, ks=ks)
            both = (st["n_pos"] > 0) & (st["n_neg"] > 0)
            assert both.all()
            want = "Val AUC: %.6f, AP: %.6f, MRR: %.6f" % (st["auc"][both].mean(), st["ap"][both].mean(), st["mrr"][both].mean())
            want += "".join(", Hits@%d: %.6f" % (k, st["hits_at"][both, i].mean()) for i, k in enumerate(ks)) + " (1 column)"
            assert line == want, (e, line, want)
