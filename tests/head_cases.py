"""The cases of tests/test_output_head.py and the procedure every one of them goes through (TEST INFRASTRUCTURE; a
module of its own because the subprocess children of that test, which set GAT_FUSE_LAST / GAT_HEAD_NODES in their own
environment, run the same procedure).

Procedure (run_case): a small context, seeded parameters, one step in the case's mode; then the head's OWN inputs are
read back through the taps (H_L and the last layer's h_pre) and handed to the fp64 reference tests/head_ref.py, and
every output of the head is compared with it: y, loss, #correct, grad_Wo, g of the last layer, gat_eval_mask.  Upstream
round-off and LeakyReLU kinks cancel (the reference uses the tapped values and signs).

Tolerances: parity.TOL absolute on y and loss / #nodes, parity.GTOL of max-abs on grad_Wo and g.  #correct must lie in
[sure, sure + |undecided|] (head_ref.py), and a case may have at most max(2, 1 %) undecided nodes.  A saturated case's
loss bar is TOL + B, B = head_ref.logit_rounding_bound (the fp32 rounding of the logits themselves).

Shapes the generic backward refuses (num_classes * D_last > 2048) stay in the sweeps: their forward is checked in full
and the step / backward must return GAT_E_UNSUPPORTED naming the output head.
"""
import dataclasses
import zlib

import numpy as np

import head_ref as hr
import parity
from parity import GTOL, TOL

SLOPE = 0.01
GAT_E_UNSUPPORTED = 10004
NLL_CLAMPED = -np.log(1e-12)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    C: int
    last: tuple = (8, 8)        # (H, D_last) of the last layer
    n: int = 200
    layers: int = 2             # 2: an (8, 8) layer in front
    in_dim: int = 12
    deg: int = 3                # mean in-degree
    mode: str = "step"          # "step": gat_step; "fwdbwd": gat_forward + gat_backward
    keep_taps: bool = False
    flat: bool = False
    dtype: str = "f32"
    masked: bool = False
    wo: str = "xavier"          # "xavier" | "saturated" | "zero" | "tie"
    hub: tuple = None           # (row, degree)
    expect_fused: bool = False  # the fused last layer must have run (GAT_FUSE_LAST=1 children)

    @property
    def heads(self):
        return ([8] if self.layers == 2 else []) + [self.last[0]]

    @property
    def outdims(self):
        return ([8] if self.layers == 2 else []) + [self.last[1]]

    @property
    def refused(self):          # the generic head backward holds grad_Wo in 8 registers of 256 threads
        return self.C * self.last[1] > 2048

    @property
    def seed(self):
        return zlib.crc32(self.name.encode()) & 0xFFFFF


def _graph(rng, n, deg, hub):
    if n == 1:
        d = np.array([1])
    elif n > 5000:
        d = np.full(n, deg)
    else:
        d = rng.integers(1, 2 * deg, n)                     # no empty rows: H_L = 0 there, a C-way tie with distinct Wo rows,
                                                            # which head_ref.py counts as undecided (Wo = 0 is the all-tie case)
    if hub is not None:
        d[hub[0]] = hub[1]
    rp = np.concatenate([[0], np.cumsum(d)]).astype(np.int32)
    dst = np.repeat(np.arange(n, dtype=np.int64), d)
    key = np.sort(dst * n + rng.integers(0, n, int(rp[-1])))  # sources ascending inside a row
    return rp, (key % n).astype(np.int32)


def _xavier(rng, case):
    F, W, a = case.in_dim, [], []
    for H, D in zip(case.heads, case.outdims):
        lim = np.sqrt(6.0 / (2 * F + D))
        W.append(rng.uniform(-lim, lim, H * D * 2 * F))
        a.append(rng.uniform(-lim, lim, H * D))
        F = H * D
    limo = np.sqrt(6.0 / (case.C + case.last[1]))
    # x 8: logits of O(1) also where H_L is small (a node whose h_pre is negative in every channel has H_L = 0.01 h_pre, and
    # with Xavier's Wo its 47 logits lie within 1e-3 of each other: top-two gaps at the undecided margin on many nodes)
    Wo = 8.0 * rng.uniform(-limo, limo, (case.C, case.last[1]))
    return np.concatenate(W).astype(np.float32), np.concatenate(a).astype(np.float32), Wo.astype(np.float32)


def make_inputs(case):
    rng = np.random.default_rng(case.seed)
    n = case.n
    rp, ci = _graph(rng, n, case.deg, case.hub)
    x = rng.standard_normal((n, case.in_dim)).astype(np.float32)
    lab = rng.integers(0, case.C, n).astype(np.int32)
    W, a, Wo = _xavier(rng, case)
    if case.wo == "zero":
        Wo[:] = 0
    mask = np.ones(n, bool)
    if case.masked:                                          # ~40 % out, node 0 and node N-1 among them
        mask = rng.random(n) > 0.4
        mask[0] = mask[-1] = False
        split = ~mask                                        # evaluation split disjoint from the training mask
    else:
        split = rng.random(n) < 1.0 / 3
        split[0] = True
    return dict(rp=rp, ci=ci, x=x, lab=lab, W=W, a=a, Wo=Wo, mask=mask, split=split, special=np.zeros(0, np.int64))


def finish_inputs(case, inp, HL):
    """The parts of a case that need H_L (which depends on neither Wo nor the labels): the power of two that saturates
    the softmax and the labels whose probability underflows; the labels of the tied classes."""
    if case.wo == "saturated":
        z0 = hr.logits(HL, inp["Wo"])
        k = int(np.ceil(np.log2(100.0 / np.abs(z0).max())))
        inp["Wo"] = (inp["Wo"] * np.float32(2.0 ** k)).astype(np.float32)        # exact
        z = z0 * 2.0 ** k
        assert 100.0 <= np.abs(z).max() <= 200.0
        spread = z.max(axis=1) - z.min(axis=1)
        nodes = np.argsort(spread)[-3:]
        # exp(-110) = 1.7e-48 is below the smallest float32 denormal: the label's probability is 0 in fp32 on any path
        nodes = nodes[spread[nodes] > 110.0]
        assert nodes.size >= 1, spread.max()
        inp["lab"][nodes] = z[nodes].argmin(axis=1)
        inp["special"] = nodes
    elif case.wo == "tie":
        Wo = inp["Wo"]
        Wo[2] = 4 * np.abs(Wo[2])                            # H_L (a mean of LeakyReLUs over mostly positive h_pre) is mostly positive
        Wo[5] = Wo[2]                                        # bit-identical and dominant
        z = hr.logits(HL, Wo)
        lead = np.nonzero(z.argmax(axis=1) == 2)[0]
        assert lead.size >= case.n // 10, lead.size
        inp["lab"][lead] = 2
        inp["lab"][lead[::4]] = 5                            # unequal counts: taking the LAST of the tie changes #correct
        inp["special"] = lead


def _expect_refusal(A, fn):
    try:
        fn()
    except A.GatError as e:
        assert e.code == GAT_E_UNSUPPORTED and "output head" in str(e), str(e)
        return
    raise AssertionError("the head backward accepted num_classes * D_last > 2048")


def _count_bounds(ref, lab, sel):
    und = np.zeros(len(lab), bool)
    und[ref.undecided] = True
    return int(((ref.pred == lab) & sel & ~und).sum()), int((und & sel).sum())


def run_case(pkg, case):
    A = pkg.abi
    inp = make_inputs(case)
    n, C = case.n, case.C
    H, DL = case.last
    L = len(case.heads) - 1
    with pkg.GatContext(case.heads, case.outdims, case.in_dim, C, keep_taps=case.keep_taps, flat_lrelu_index=case.flat,
                        dtype=case.dtype, collect_timing=case.expect_fused) as ctx:
        ctx.set_graph(inp["rp"], inp["ci"]); ctx.set_features(inp["x"]); ctx.set_labels(inp["lab"])
        ctx.params_set(A.PARAM_W, inp["W"]); ctx.params_set(A.PARAM_A, inp["a"]); ctx.params_set(A.PARAM_WO, inp["Wo"])
        if case.wo in ("saturated", "tie"):
            ctx.forward(want_loss=False)
            finish_inputs(case, inp, ctx.tap(A.TAP_HOUT, L))
            ctx.set_labels(inp["lab"]); ctx.params_set(A.PARAM_WO, inp["Wo"])
        lab, mask, split, Wo = inp["lab"], inp["mask"], inp["split"], inp["Wo"]
        if case.masked:
            ctx.set_train_mask(mask)
        ctx.zero_grad()
        if case.mode == "step":
            if case.refused:
                _expect_refusal(A, ctx.step)
                loss, correct = ctx.forward()               # the context is still usable after the refusal
            else:
                loss, correct = ctx.step()
        else:
            loss, correct = ctx.forward()
            if case.refused:
                _expect_refusal(A, ctx.backward)
            else:
                ctx.backward()
        if case.expect_fused:
            assert "GAT_FUSE_LAST=1" in A.switches(), A.switches()
            name = ctx.lib.gat_kernel_name(A.K_EDGE_FUSED).decode()
            assert ctx.kernel_stats()[name][0] > 0, "the fused last layer did not run"

        HL = ctx.tap(A.TAP_HOUT, L)
        hpre = ctx.tap(A.TAP_HPRE, L)
        ref = hr.head_ref(HL, hpre, Wo, lab, mask, H, SLOPE, case.flat)
        cap = max(2.0, 0.01 * n)
        parity.record("undecided", len(ref.undecided), cap)
        assert len(ref.undecided) <= cap, (len(ref.undecided), cap)
        y = ctx.tap(A.TAP_Y)
        assert np.isfinite(y).all()
        n_train = int(mask.sum())
        el, ec, en = ctx.eval_mask(split)
        gWo = g = None
        if not case.refused:
            gWo = ctx.grads_get(A.PARAM_WO).reshape(C, DL)
            g = ctx.tap(A.TAP_G, L)

        if C == 1:                                           # one class: y == 1, no loss, no gradient — exactly
            assert np.all(y == 1.0) and loss == 0.0 and correct == n_train
            assert not gWo.any() and not g.any()
            assert (el, ec, en) == (0.0, int(split.sum()), int(split.sum()))
            return
        parity.check_abs("y", y, ref.y)
        B = hr.logit_rounding_bound(HL[mask], Wo) if case.wo == "saturated" else 0.0
        err = abs(loss - ref.nll[mask].sum()) / n_train
        parity.record("loss/n", err, TOL + B, B=B)
        assert err <= TOL + B, (err, TOL, B)
        sure, slack = _count_bounds(ref, lab, mask)
        parity.record("n_correct - sure", correct - sure, slack)
        assert sure <= correct <= sure + slack, (correct, sure, slack)

        assert en == int(split.sum())
        Bs = hr.logit_rounding_bound(HL[split], Wo) if case.wo == "saturated" else 0.0
        err = abs(el - ref.nll[split].sum()) / en
        parity.record("eval loss/n", err, TOL + Bs, B=Bs)
        assert err <= TOL + Bs, (err, TOL, Bs)
        sure, slack = _count_bounds(ref, lab, split)
        assert sure <= ec <= sure + slack, (ec, sure, slack)

        if not case.refused:
            parity.check_rel("gradWo", gWo, ref.gradWo)
            parity.check_rel("g", g, ref.g)
            if case.masked:
                assert not g[~mask].any()                    # dz is exactly 0 outside the training mask

        if case.wo == "saturated":
            assert (y == 0).any()
            for node in inp["special"]:                      # the label's probability underflowed: the 1e-12 clamp, alone
                assert y[node, lab[node]] == 0.0 and ref.nll[node] == NLL_CLAMPED
                one = np.zeros(n, bool)
                one[node] = True
                l1, _, n1 = ctx.eval_mask(one)
                # logf of the float32 nearest 1e-12: 4 ulp of 27.6 in fp32 is 7.6e-6
                assert n1 == 1 and abs(l1 - NLL_CLAMPED) <= 1e-5, (l1, NLL_CLAMPED)
        if case.wo in ("zero", "tie"):                       # exact ties are decided: the first maximum wins
            assert len(ref.undecided) == 0
            assert correct == int(((ref.pred == lab) & mask).sum())
            if case.wo == "zero":
                assert not ref.pred.any() and correct == int((lab[mask] == 0).sum())
            else:
                lead = inp["special"]
                assert np.all(ref.pred[lead] == 2) and np.all(y[lead, 2] == y[lead, 5])


# ---- the cases ----------------------------------------------------------------------------------------------------
def _c_sweep():
    out = []
    for c in (1, 2, 3, 40, 47, 63, 64, 65, 100, 255, 256, 257, 300):
        out.append(Case(f"C{c}", c, (8, 8)))                 # C = 257 and 300: 2056 and 2400 > 2048, the backward is refused
    out.append(Case("C257-d4", 257, (8, 4)))                 # ... so the whole head at those C runs at D_last = 4
    out.append(Case("C300-d4", 300, (8, 4)))                 # NB = 32, per_thread = 5
    return out


D_SHAPES = [(8, 4), (8, 8), (4, 16), (2, 32), (1, 64), (1, 2), (1, 5), (1, 12), (1, 24), (1, 33), (1, 100)]


def _d_sweep():
    return [Case(f"C{c}-h{h}d{d}", c, (h, d), layers=1, in_dim=10) for c in (7, 47) for h, d in D_SHAPES]


def _n_sweep():
    out = [Case(f"N{n}", 7, (8, 8), n=n) for n in (1, 127, 128, 129, 257)]
    # more tiles than blocks (the head's grids stop at 1024 blocks of 128 nodes) and a ragged last tile
    out.append(Case("N140001", 7, (8, 8), n=140001, layers=1, in_dim=4, deg=2))
    return out


def _modes():
    out = []
    for c, last, layers in ((3, (8, 8), 2), (47, (8, 8), 2), (64, (8, 8), 2), (65, (8, 8), 2), (256, (8, 8), 2), (257, (8, 4), 2),
                            (7, (4, 16), 1), (7, (1, 5), 1), (47, (1, 33), 1), (7, (1, 100), 1), (47, (1, 64), 1)):
        tag = f"C{c}-h{last[0]}d{last[1]}"
        kw = dict(layers=layers, in_dim=12 if layers == 2 else 10)
        out.append(Case(f"fwdbwd-{tag}", c, last, mode="fwdbwd", **kw))
        out.append(Case(f"taps-{tag}", c, last, keep_taps=True, **kw))
        out.append(Case(f"flat-{tag}", c, last, flat=True, mode="fwdbwd" if c % 2 else "step", **kw))
    for c, last in ((7, (8, 8)), (47, (4, 16)), (7, (1, 64)), (63, (2, 32)), (100, (8, 4))):
        out.append(Case(f"bf16-C{c}-h{last[0]}d{last[1]}", c, last, dtype="bf16"))
    for c, last, n in ((7, (8, 8), 200), (64, (8, 8), 257), (65, (8, 8), 129), (300, (8, 4), 200), (47, (1, 12), 200)):
        for mode in ("step", "fwdbwd"):
            out.append(Case(f"mask-{mode}-C{c}-h{last[0]}d{last[1]}", c, last, n=n, mode=mode, masked=True,
                            layers=1 if last[0] == 1 else 2, in_dim=10 if last[0] == 1 else 12))
    out.append(Case("mask-flat-C7", 7, (8, 8), flat=True, masked=True))
    out.append(Case("mask-taps-C65", 65, (8, 8), keep_taps=True, masked=True))
    return out


def _special():
    out = []
    for mode in ("step", "fwdbwd"):
        out.append(Case(f"saturated-{mode}-C7", 7, (8, 8), mode=mode, wo="saturated"))
        out.append(Case(f"saturated-{mode}-C100", 100, (8, 8), mode=mode, wo="saturated"))
        out.append(Case(f"zero-{mode}-C7", 7, (8, 8), mode=mode, wo="zero"))
        out.append(Case(f"tie-{mode}-C7", 7, (8, 8), mode=mode, wo="tie"))
    out.append(Case("zero-C65", 65, (8, 8), wo="zero"))
    out.append(Case("tie-C65", 65, (8, 8), wo="tie"))
    return out


CASES = _c_sweep() + _d_sweep() + _n_sweep() + _modes() + _special()

# children: the switches are read once per process.  The fused last layer needs (H, D_last) = (8, 8), C <= 64, fp32; the hub
# row (beyond one 16-edge segment) makes head_rows_kernel run for it.
_FUSED = [Case(f"fused-C{c}{'-mask' if m else ''}", c, (8, 8), hub=(5, 70), masked=m, expect_fused=True)
          for c, m in ((1, False), (7, False), (7, True), (47, False), (64, True))]
_FUSED += [Case("fused-tie-C7", 7, (8, 8), hub=(5, 70), wo="tie", expect_fused=True),
           Case("fused-saturated-C7", 7, (8, 8), hub=(5, 70), wo="saturated", expect_fused=True)]
_NODES256 = [Case(f"nodes256-{mode}-C{c}-N{n}", c, (8, 8), n=n, mode=mode, deg=2)
             for c, n in ((7, 257), (47, 513), (65, 300), (257, 129)) for mode in ("step", "fwdbwd")]
CHILDREN = {
    "GAT_FUSE_LAST=1": ({"GAT_FUSE_LAST": "1"}, _FUSED),
    "GAT_HEAD_NODES=256": ({"GAT_HEAD_NODES": "256"}, _NODES256),
    "GAT_FUSE_LAST=1 GAT_HEAD_NODES=256": ({"GAT_FUSE_LAST": "1", "GAT_HEAD_NODES": "256"},
                                           [dataclasses.replace(c, name="both-" + c.name) for c in _FUSED[1:4]]),
}
BY_NAME = {c.name: c for c in CASES + [c for _, cs in CHILDREN.values() for c in cs]}
assert len(BY_NAME) == len(CASES) + sum(len(cs) for _, cs in CHILDREN.values())
