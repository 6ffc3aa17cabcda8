"""Negative sampling on the GPU (include/gatv2_abi.h "negative sampling"): the sampler through its stateless seam, bitwise against
synth.negative_pairs; a resample on a context — the drawn pairs, the slots outside, the info, and the step after it bitwise that of a
fresh context given the same lists through set_pairs (so the device-built work list is the host's), also across a captured replay and
with a node cut into three segments; two cases against the fp64 model of tests/pair_ref.py at 1e-4; the state and refusal matrix; the
train_edge host.

tests/test_neg_sampling_cpu.py proves on the host that the reference obeys the law and that the ascending fixture has no unfiltered
negative in UNIFORM mode at any (count, round) used here."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import feature_cases as FC
import neg_cases as NC
import pair_ref as PR
import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
E_INVALID, E_STATE = 10001, 10002
SENTINEL = -7
D8 = ("records_d8", [8, 8], [8, 8], {})


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the seam tests need the GPU"
    return torch, torch.device("cuda:0")


def to_dev(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev) if len(a) else torch.zeros(1, dtype=torch.int32, device=dev)


def seam(pkg, torch_dev, d_rp, d_ci, n, e, mode, flags, seed, rnd, count, su=None, sv=None):
    """One gat_op_negative_sample call -> (u, v, unfiltered); one entry of padding behind the outputs stays untouched."""
    torch, dev = torch_dev
    d_u = torch.full((count + 1,), SENTINEL, dtype=torch.int32, device=dev)
    d_v = torch.full((count + 1,), SENTINEL, dtype=torch.int32, device=dev)
    kw = {}
    if su is not None:
        d_su, d_sv = to_dev(torch, dev, su), to_dev(torch, dev, sv)
        kw = dict(d_src_u=d_su.data_ptr(), d_src_v=d_sv.data_ptr(), n_src=len(su))
    unf = pkg.abi.op_negative_sample(d_rp.data_ptr(), d_ci.data_ptr() if e else 0, n, e, mode, flags, seed, rnd, d_u.data_ptr(), d_v.data_ptr(),
                                     count, **kw)
    u, v = d_u.cpu().numpy(), d_v.cpu().numpy()
    assert u[count] == SENTINEL and v[count] == SENTINEL
    return u[:count], v[:count], unf


def same(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (what, got[2], want[2])


# -- the seam
@pytest.mark.parametrize("mode", (NC.UNIFORM, NC.CORRUPT))
@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_seam_is_the_reference_bitwise(pkg, torch_dev, variant, mode):
    torch, dev = torch_dev
    rp, ci = NC.fixture_graph(pkg, variant)
    d_rp, d_ci = to_dev(torch, dev, rp), to_dev(torch, dev, ci)
    su, sv = NC.sources(pkg, rp, ci) if mode == NC.CORRUPT else (None, None)
    kw = dict(src_u=su, src_v=sv) if mode == NC.CORRUPT else {}
    for flags in NC.FLAGS:
        for count in NC.COUNTS:
            for rnd in NC.ROUNDS:
                want = pkg.synth.negative_pairs(rp, ci, mode, count, NC.SEED, rnd, flags, **kw)
                got = seam(pkg, torch_dev, d_rp, d_ci, NC.N, len(ci), mode, flags, NC.SEED, rnd, count, su, sv)
                same(got, want, (flags, count, rnd))
                if mode == NC.UNIFORM and variant == "ascending":
                    assert got[2] == 0                   # (the CPU twin's condition: the filter, not the fall-back, was compared)
    assert np.array_equal(d_ci.cpu().numpy(), ci) and np.array_equal(d_rp.cpu().numpy(), rp)        # the graph is untouched


def test_seam_exhaustion_and_degenerate_graphs(pkg, torch_dev):
    torch, dev = torch_dev
    rp, ci = NC.fixture_graph(pkg, "ascending")
    d_rp, d_ci = to_dev(torch, dev, rp), to_dev(torch, dev, ci)
    su, sv = NC.hub_sources()                            # role 0 replaces the source: (w, hub) is an edge on every attempt
    for flags in NC.FLAGS:
        want = pkg.synth.negative_pairs(rp, ci, NC.CORRUPT, 1000, NC.SEED, 1, flags, src_u=su, src_v=sv)
        assert want[2] > 300
        same(seam(pkg, torch_dev, d_rp, d_ci, NC.N, len(ci), NC.CORRUPT, flags, NC.SEED, 1, 1000, su, sv), want, ("hub", flags))
    rp, ci = NC.complete_graph(4)
    d_rp, d_ci = to_dev(torch, dev, rp), to_dev(torch, dev, ci)
    s2u, s2v = np.array([0, 1], np.int32), np.array([2, 3], np.int32)
    for flags in NC.FLAGS:
        for count in NC.COUNTS:
            want = pkg.synth.negative_pairs(rp, ci, NC.UNIFORM, count, NC.SEED, 2, flags)
            assert want[2] == count
            same(seam(pkg, torch_dev, d_rp, d_ci, 4, len(ci), NC.UNIFORM, flags, NC.SEED, 2, count), want, ("K4", flags, count))
        want = pkg.synth.negative_pairs(rp, ci, NC.CORRUPT, 65, NC.SEED, 2, flags, src_u=s2u, src_v=s2v)
        same(seam(pkg, torch_dev, d_rp, d_ci, 4, len(ci), NC.CORRUPT, flags, NC.SEED, 2, 65, s2u, s2v), want, ("K4 corrupt", flags))
    rp, ci = NC.single_node()
    d_rp, d_ci = to_dev(torch, dev, rp), to_dev(torch, dev, ci)
    for flags in NC.FLAGS:
        want = pkg.synth.negative_pairs(rp, ci, NC.UNIFORM, 65, NC.SEED, 0, flags)
        assert want[2] == (0 if flags & NC.SELF else 65)
        same(seam(pkg, torch_dev, d_rp, d_ci, 1, 0, NC.UNIFORM, flags, NC.SEED, 0, 65), want, ("N1", flags))


def test_seam_refusals(pkg, torch_dev):
    A = pkg.abi
    torch, dev = torch_dev
    rp, ci = NC.fixture_graph(pkg, "ascending")
    d_rp, d_ci = to_dev(torch, dev, rp), to_dev(torch, dev, ci)
    d_u = torch.zeros(8, dtype=torch.int32, device=dev); d_v = torch.zeros(8, dtype=torch.int32, device=dev)
    d_su = torch.tensor([1, 2, NC.N], dtype=torch.int32, device=dev); d_sv = torch.tensor([3, 4, 5], dtype=torch.int32, device=dev)
    bad_rp = rp.copy(); bad_rp[-1] += 1
    d_bad = to_dev(torch, dev, bad_rp)
    e = len(ci)

    def call(rp_=d_rp, mode=NC.UNIFORM, flags=0, count=8, **kw):
        return A.op_negative_sample(rp_.data_ptr(), d_ci.data_ptr(), NC.N, e, mode, flags, 1, 0, d_u.data_ptr(), d_v.data_ptr(), count, **kw)

    for fn, text in ((lambda: call(mode=0), "mode"), (lambda: call(mode=3), "mode"), (lambda: call(flags=4), "flag"), (lambda: call(count=0), "sizes"),
                     (lambda: call(mode=NC.CORRUPT), "source pair"),
                     (lambda: call(mode=NC.CORRUPT, d_src_u=d_su.data_ptr(), d_src_v=d_sv.data_ptr(), n_src=3), f"pair 2 has u {NC.N} outside"),
                     (lambda: call(rp_=d_bad), "row_ptr")):
        with pytest.raises(A.GatError) as ei:
            fn()
        assert ei.value.code == E_INVALID and text in str(ei.value), str(ei.value)
    torch.cuda.synchronize()
    assert call() == 0


# -- the context
def all_grads(A, c):
    return [c.grads_get(k) for k in A.PARAM_GROUPS]


def with_pairs(ci, u, v):
    """The case on another pair list (any length): softmax labels per pair."""
    return dict(ci, u=np.asarray(u, np.int32), v=np.asarray(v, np.int32), sup=PR.pair_labels(len(u), ci["g"]["c"]), mask=None)


def expected_pairs(pkg, ci, mode, first, count, flags, seed, rnd):
    """The reference applied to the context's graph."""
    g = ci["g"]
    kw = dict(src_u=ci["u"][:first], src_v=ci["v"][:first]) if mode == NC.CORRUPT else {}
    nu, nv, unf = pkg.synth.negative_pairs(g["row_ptr"], g["col_idx"], mode, count, seed, rnd, flags, **kw)
    u, v = ci["u"].copy(), ci["v"].copy()
    u[first:first + count], v[first:first + count] = nu, nv
    return u, v, unf


def check_resample(pkg, ci, live, mode, first, count, flags, seed, rnd):
    """resample_negatives(rnd) on `live`: pairs(), the info, and the step bitwise that of a fresh context with the same lists."""
    A = pkg.abi
    live.resample_negatives(rnd)
    u, v, unf = expected_pairs(pkg, ci, mode, first, count, flags, seed, rnd)
    gu, gv = live.pairs()
    assert np.array_equal(gu, u) and np.array_equal(gv, v), (mode, rnd)
    assert live.negatives_info() == (mode, first, count, rnd, unf)
    with PR.make_ctx(pkg, ci, u=u, v=v) as fresh:
        want = fresh.step(); gw = all_grads(A, fresh)
    live.zero_grad()
    assert live.step() == want, (mode, rnd)
    for k in A.PARAM_GROUPS:
        assert np.array_equal(live.grads_get(k), gw[k]), (mode, rnd, k)
    return want, gw, (u, v)


@pytest.mark.parametrize("mode,first,count,flags", [(NC.UNIFORM, 200, 202, 0), (NC.CORRUPT, 200, 202, NC.BOTH), (NC.UNIFORM, 100, 150, NC.SELF)],
                         ids=["uniform", "corrupt-both", "uniform-inner-slots"])
def test_resample_on_a_context(pkg, orc, mode, first, count, flags):
    A = pkg.abi
    ci = PR.case_inputs((*D8, "plain", "mul", PR.SOFTMAX))
    assert first + count <= len(ci["u"])
    both, allow = bool(flags & NC.BOTH), bool(flags & NC.SELF)
    with PR.make_ctx(pkg, ci) as live, PR.make_ctx(pkg, ci) as cap:
        live.set_negative_sampling(mode, first, count, both_directions=both, allow_self=allow, seed=NC.SEED)
        assert live.negatives_info() == (mode, first, count, 0, 0)
        gu, gv = live.pairs()
        assert np.array_equal(gu, ci["u"]) and np.array_equal(gv, ci["v"])       # it draws nothing itself
        for rnd in (0, 5, 2 ** 40):
            want, gw, (u, v) = check_resample(pkg, ci, live, mode, first, count, flags, NC.SEED, rnd)
        cap.set_negative_sampling(mode, first, count, both_directions=both, allow_self=allow, seed=NC.SEED)
        cap.step_graph(True)
        for _ in range(3):                               # warm-up, capture + replay, replay: on the first pairs
            cap.zero_grad()
            cap.step()
        cap.resample_negatives(2 ** 40)                  # re-arms: eager, capture + replay, replay on the drawn pairs
        for _ in range(3):
            cap.zero_grad()
            assert cap.step() == want
            for k in A.PARAM_GROUPS:
                assert np.array_equal(cap.grads_get(k), gw[k]), k


def test_resample_cuts_a_node_into_segments(pkg, orc):
    """CORRUPT with count = 1200 and every source ending at one node: its incidences cross 256 and 512, the device plan's split path."""
    base = PR.case_inputs((*D8, "plain", "mul", PR.SOFTMAX))
    n = base["g"]["n"]
    first, count, shared = 50, 1200, 20
    u0 = np.concatenate([(np.arange(first) * 3 + 1) % n, np.zeros(count, np.int64)])
    v0 = np.concatenate([np.full(first, shared), np.zeros(count, np.int64)])
    ci = with_pairs(base, u0, v0)
    with PR.make_ctx(pkg, ci) as live:
        live.set_negative_sampling(NC.CORRUPT, first, count, seed=NC.SEED)
        for rnd in (1, 2):
            _, _, (u, v) = check_resample(pkg, ci, live, NC.CORRUPT, first, count, 0, NC.SEED, rnd)
            inc = np.bincount(u, minlength=n) + np.bincount(v, minlength=n)
            assert inc[shared] > 512 and np.sum(inc > 256) >= 1


# -- fp64
TAPS = ["hout", "G"]


@pytest.mark.parametrize("pair_mode,loss", [("mul", PR.BCE), ("add", PR.MSE)])
def test_step_after_a_resample_against_fp64(pkg, orc, pair_mode, loss):
    import loss_ref as LR
    A = pkg.abi
    ci = PR.case_inputs((*D8, "plain", pair_mode, loss))
    P = len(ci["u"])
    with PR.make_ctx(pkg, ci) as ctx:
        ctx.set_negative_sampling("uniform", 200, P - 200, both_directions=True, seed=NC.SEED)
        ctx.resample_negatives(3)
        u, v = ctx.pairs()
        assert not np.array_equal(u[200:], ci["u"][200:])
        ref = PR.model_of(ci, u, v)
        loss_sum, _ = ctx.step()
        rows = max(1, int(LR.contributes(ci["sup"], ci["mask"]).sum()))
        FC.compare(pkg, ctx, dict(ci["g"], n=rows), ci["cfg"], ref, loss_sum, 1e-4, TAPS, FC.GROUPS[:7])
        parity.check_rel("paired", ctx.tap(A.TAP_PAIRED, ci["cfg"].L - 1), ref["paired"].detach().numpy(), 1e-4)
        parity.check_abs("y", ctx.tap(A.TAP_Y), ref["y"], 1e-4)


# -- states and refusals
def test_state_and_refusal_matrix(pkg, orc):
    A = pkg.abi
    ci = PR.case_inputs((*D8, "plain", "mul", PR.SOFTMAX))
    g = ci["g"]
    P = len(ci["u"])

    def refused(code, fn, text=None):
        with pytest.raises(A.GatError) as ei:
            fn()
        assert ei.value.code == code, str(ei.value)
        if text is not None:
            assert text in str(ei.value), str(ei.value)

    with pkg.GatContext([8, 8], [8, 8], g["f"], g["c"]) as c:            # no pair head
        c.set_graph(g["row_ptr"], g["col_idx"])
        refused(E_STATE, lambda: c.set_negative_sampling("uniform", 0, 1), "pair head")
        refused(E_STATE, lambda: c.resample_negatives(0), "gat_set_negative_sampling comes first")
        refused(E_STATE, lambda: c.pairs(), "pair head")
        c.set_negative_sampling("none")                                  # off is always accepted
        assert c.negatives_info() == (0, 0, 0, 0, 0)
    with PR.make_ctx(pkg, ci) as c, PR.make_ctx(pkg, ci) as plain:
        want = plain.step(); gw = all_grads(A, plain)
        refused(E_STATE, lambda: c.resample_negatives(0))                # before gat_set_negative_sampling
        for args in ((3, 0, 1), (-1, 0, 1), ("uniform", 0, 0), ("uniform", -1, 2), ("uniform", P, 1), ("uniform", 1, P), ("corrupt", 0, 5)):
            refused(E_INVALID, lambda: c.set_negative_sampling(*args))
        refused(E_INVALID, lambda: A._chk(c.lib.gat_set_negative_sampling(c._ctx, 1, 0, 1, 4, 0)), "flag")
        buf = np.zeros(P + 1, np.int32)
        refused(E_INVALID, lambda: A._chk(c.lib.gat_pairs_get(c._ctx, buf.ctypes.data_as(ctypes.c_void_p), buf.ctypes.data_as(ctypes.c_void_p), P + 1)), "n_pairs")
        assert c.negatives_info() == (0, 0, 0, 0, 0)                     # nothing stuck
        c.set_negative_sampling("uniform", 0, P)                         # the whole list, and then off again without a draw:
        c.set_negative_sampling("none")
        refused(E_STATE, lambda: c.resample_negatives(0))
        assert c.step() == want                                          # bitwise a context that never used the feature
        for k in A.PARAM_GROUPS:
            assert np.array_equal(c.grads_get(k), gw[k]), k
        c.set_negative_sampling("corrupt", 100, P - 100, seed=3)         # used, then off: the pairs stay what was drawn
        c.resample_negatives(7)
        u, v = c.pairs()
        c.set_negative_sampling(0)
        assert c.negatives_info() == (0, 0, 0, 0, 0)
        refused(E_STATE, lambda: c.resample_negatives(8))
        gu, gv = c.pairs()
        assert np.array_equal(gu, u) and np.array_equal(gv, v)
        with PR.make_ctx(pkg, ci, u=u, v=v) as never:
            want2 = never.step(); gw2 = all_grads(A, never)
        c.zero_grad()
        assert c.step() == want2
        for k in A.PARAM_GROUPS:
            assert np.array_equal(c.grads_get(k), gw2[k]), k


# -- the host program
def run_host(root, seed, epochs=3):
    env = dict(os.environ)
    env.pop("DATA_ROOT", None)
    r = subprocess.run([BIN, "--dataset", "tiny", "--data-root", root, "--epochs", str(epochs), "--optimizer", "adam", "--lr", "0.01", "--clip",
                        "--num-layers", "2", "--heads", "8,8", "--outdims", "8,8", "--seed", "7", "--pairs", "mul", "--loss", "bce",
                        "--neg-sampling", "uniform", "--neg-first", "60", "--neg-seed", str(seed), "--neg-both-directions"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = re.findall(r"Avg Loss: ([0-9.]+), Accuracy: ([0-9.]+)%", r.stdout)
    assert len(got) == epochs, r.stdout
    return got, r.stdout


def test_train_edge_negative_sampling(pkg, orc):
    """train_edge --pairs mul --loss bce --neg-sampling uniform: the same seed prints the same epochs, another seed others, and the
    epochs match a GatContext that resamples with round = the epoch's number before each forward."""
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
        x = np.loadtxt(os.path.join(d, "features.txt"), dtype=np.float32, ndmin=2)      # exactly what the binary reads
        a, out = run_host(root, 5)
        b, _ = run_host(root, 5)
        c, _ = run_host(root, 6)
        assert f"Negative sampling: uniform, pairs 60 .. {P - 1} redrawn before every epoch\n" in out
        assert a == b and [l for l, _ in a] != [l for l, _ in c]
    with pkg.GatContext([8, 8], [8, 8], g["f"], 1) as ctx:
        ctx.set_loss("bce")
        ctx.set_graph(g["row_ptr"], g["col_idx"]); ctx.set_features(x)
        ctx.set_pairs("mul", u, v)
        ctx.set_targets(t.reshape(P, 1))
        ctx.params_init(7)
        ctx.set_negative_sampling("uniform", 60, P - 60, both_directions=True, seed=5)
        ctx.zero_grad()
        for e, (loss_txt, acc_txt) in enumerate(a, 1):
            ctx.resample_negatives(e)
            loss, correct = ctx.forward()
            ctx.backward()
            ctx.clip(5.0)
            ctx.step_adam(0.01, 0.9, 0.999, 1e-8, e)
            ctx.zero_grad()
            assert loss_txt == "%f" % (np.float32(loss) / P), (e, loss_txt, loss / P)
            assert acc_txt == "%.2f" % (100.0 * np.float32(np.float32(correct) / P)), (e, acc_txt, correct)
