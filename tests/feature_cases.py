"""What the feature tests share (tests/test_dropout.py, test_dropedge.py, test_residual.py, test_norm.py, test_edge_shapes.py and their
_cpu twins): the graphs, the dispatcher families, the regulariser masks, the case table of the edge shapes, the context builder, the
seed search against the fp64 model of tests/step_ref.py, the comparison of a context with that model, and the shard worker.  A plain
module: the test modules import it, never each other."""
import itertools
import os
import sys

import numpy as np

import dropedge_ref as E
import dropout_ref as R
import parity
import step_ref as SR
from conftest import small_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUPS = SR.GROUPS                               # the ten parameter groups in the ABI's order; the call sites slice it
EPS = 1e-5

FAMILIES = [
    ("records_d8", [8, 8], [8, 8], {}),
    ("records_d4", [16, 16], [4, 4], {}),
    ("msg_rows_d16", [4, 4], [16, 16], {}),
    ("hd16", [2, 2], [8, 8], {}),
    ("generic", [3, 2], [5, 8], {}),
    ("hd128_generic", [16, 2], [8, 8], {}),
    ("keep_taps", [8, 8], [8, 8], {"keep_taps": True}),
    ("bf16", [8, 8], [8, 8], {"dtype": "bf16"}),
]
# (name, GAT_RES_LINEAR, GAT_RES_BIAS)
RES_MODES = [("linear", True, False), ("bias", False, True), ("both", True, True)]
NORM_MODES = [("norm", False, False), ("norm_res", True, True)]
REG = dict(pe=0.4, pa=0.3, pf=0.5, seed=78)      # the three regularisers of the "all on" runs


def make_graph(seed, n=300, e=4000, F=24, C=5, self_loops=False):
    """A graph with an empty row and a hub row of 300 in-edges (split into segments: its edge positions span them).
    self_loops: the first edge of every non-empty row is replaced by the row's self-loop."""
    rng = np.random.default_rng(seed)
    rp, ci = small_graph(rng, n, e, hub=(7, 300), empty=(3,))
    if self_loops:
        ne = np.diff(rp) > 0
        ci = ci.copy()
        ci[rp[:-1][ne]] = np.arange(n, dtype=np.int32)[ne]
    x = rng.standard_normal((n, F)).astype(np.float32)
    lab = rng.integers(0, C, n).astype(np.int32)
    return dict(row_ptr=rp, col_idx=ci, x=x, labels=lab, n=n, f=F, c=C)


def parity_graph():
    """make_graph with the hub row (300 in-edges, segments) and the empty row kept, but 150 nodes / 700 other edges: with 4000 edges x
    64 channels hardly any Xavier seed keeps every |s| above 1e-5."""
    return make_graph(5, n=150, e=700)


def wide_graph():
    """40 nodes, 200 edges, F = 12, one empty row: with 260 channels a larger graph leaves no seed clear of the kinks."""
    rng = np.random.default_rng(9)
    rp, ci = small_graph(rng, 40, 200, empty=(3,))
    return dict(row_ptr=rp, col_idx=ci, x=rng.standard_normal((40, 12)).astype(np.float32), labels=rng.integers(0, 4, 40).astype(np.int32),
                n=40, f=12, c=4)


def host_graph(seed, n=40, e=300, F=6, C=3):
    """The graph of the models' own host tests: a hub row (7) of 40 in-edges, one empty row (3)."""
    rng = np.random.default_rng(seed)
    rp, ci = small_graph(rng, n, e, hub=(7, 40), empty=(3,))
    x = rng.standard_normal((n, F)).astype(np.float32)
    lab = rng.integers(0, C, n).astype(np.int32)
    return dict(row_ptr=rp, col_idx=ci, x=x, labels=lab, n=n, f=F, c=C)


# rows wider than one round of the norm backward kernel's row lanes: H*D = 65 (not a multiple of 4: one channel per lane, 64 lanes, two
# rounds) and H*D = 260 (four channels per lane, two rounds); both on the generic edge kernels
WIDE = [("hd65", [5, 2], [13, 8]), ("hd260", [20, 2], [13, 8])]

ROWS_PE, ROWS_SEED = 0.9, 1


def rows_keeps(g):
    """DropEdge at p_e = 0.9: masks that empty non-empty rows."""
    return [E.edge_keep(ROWS_SEED, 1, l, g["row_ptr"], g["col_idx"], ROWS_PE) for l in range(2)]


def masks(cfg, g, heads, reg):
    """(keeps, attn, feat) of step 1 for the regularisers in reg (None: plain)."""
    if reg is None:
        return None, None, None
    keeps = [E.edge_keep(reg["seed"], 1, l, g["row_ptr"], g["col_idx"], reg["pe"]) for l in range(cfg.L)]
    attn = [R.attn_factor(reg["seed"], 1, l, g["row_ptr"], heads[l], reg["pa"]) for l in range(cfg.L)]
    feat = [R.feat_factor(reg["seed"], 1, l, g["n"], cfg.in_dims[l], reg["pf"]) for l in range(cfg.L)]
    return keeps, attn, feat


# -- the case table of tests/test_edge_shapes.py
SHAPES = [(64, 8), (64, 4), (64, 16), (64, 32), (64, 64), (32, 8), (32, 4), (32, 16), (32, 32), (16, 4), (16, 8), (16, 16), (8, 4), (8, 8)]
DTYPES = ["fp32", "bf16"]
# form -> (set_norm + set_residual(linear, bias), the three regularisers of REG, keep_taps)
FORMS = {
    "reg": (False, True, False),
    "res_norm": (True, False, False),
    "res_norm_reg": (True, True, False),
    "taps_res_norm_reg": (True, True, True),
}
CASES = [(hd, d, dt, form) for (hd, d), dt, form in itertools.product(SHAPES, DTYPES, FORMS)]


def case_id(case):
    hd, d, dt, form = case
    return f"hd{hd}_d{d}-{dt}-{form}"


def shape_model(orc, hd, d):
    """A shape (HD, D) is the two-layer model heads [H, H], outdims [D, D], H = HD / D, on parity_graph."""
    h = hd // d
    g = parity_graph()
    return g, [h, h], [d, d], orc.Config([h, h], [d, d], g["f"], g["c"])


def pick_shape(orc, cfg, g, norm, reg, bf16):
    """The parameters of an edge-shape case.  With the norm: norm + both residual flags at the bounds of tests/test_norm.py (|s| > 1e-5,
    |v| > 1e-4).  Without: the plain regularised model, v = h_pre, at the bounds of tests/test_residual.py (|s| > 1e-5, |h_pre| > 1e-5)."""
    if norm:
        return pick_case(orc, cfg, g, NORM_MODES[1], norm=True, reg=reg, bf16_pl=bf16)
    return pick_case(orc, cfg, g, None, reg=reg, bf16_pl=bf16, clear=clear_of(s=1e-5, v=1e-5))


# -- contexts
def make_ctx(pkg, g, heads, outdims, P, *, Wres=None, b=None, gamma=None, beta=None, residual=None, norm=None, reg=None, **kw):
    """A context on graph g with the given parameter groups set and its gradients zeroed.  norm: keyword arguments of set_norm, residual:
    (linear, bias) of set_residual (None: the call is not made), both before the graph as the ABI requires; reg: the regularisers (REG's
    keys), set after the parameters.  **kw goes to GatContext."""
    ctx = pkg.GatContext(heads, outdims, g["f"], g["c"], **kw)
    if norm is not None:
        ctx.set_norm(**norm)
    if residual is not None:
        ctx.set_residual(linear=residual[0], bias=residual[1])           # after gat_set_norm: either order is allowed
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    ctx.set_labels(g["labels"])
    for grp, arr in enumerate((*P, Wres, b, gamma, beta)):
        if arr is not None:
            ctx.params_set(grp, arr)
    if reg is not None:
        ctx.set_dropout(reg["pf"], reg["pa"], seed=reg["seed"], first_step=0)
        ctx.set_dropedge(reg["pe"])
    ctx.zero_grad()
    return ctx


def setters(mode, norm=False, skip_last=False):
    """make_ctx's residual= and norm= of a mode (name, linear, bias): gat_set_residual is called where a flag is on."""
    return dict(residual=mode[1:] if mode[1] or mode[2] else None, norm=dict(skip_last=skip_last, eps=EPS) if norm else None)


def grads(pkg, ctx, groups):
    """The gradient groups named in groups (names of GROUPS)."""
    A = pkg.abi
    ids = dict(zip(GROUPS, (A.PARAM_W, A.PARAM_A, A.PARAM_WO, A.PARAM_WRES, A.PARAM_B, A.PARAM_LN_G, A.PARAM_LN_B, A.PARAM_WE, A.PARAM_HEAD_W,
                             A.PARAM_HEAD_B)))
    return [ctx.grads_get(ids[k]) for k in groups]


# -- the seed search
def clear_of(s, hpre=None, v=None):
    """-> the predicate "every non-zero |s|, |h_pre|, |v| of the model's outputs is above its bound" (None: not looked at)."""
    def clear(ref):
        return ref["s_min"] > s and (hpre is None or ref["hpre_min"] > hpre) and (v is None or ref["v_min"] > v)
    return clear


CLEAR_HPRE = clear_of(s=1e-5, hpre=1e-5)         # the dropout, DropEdge and residual cases
CLEAR_V = clear_of(s=1e-5, v=1e-4)               # the norm cases


def pick_params(orc, cfg, model, clear):
    """First Xavier seed ps (of 40) whose fp64 model is clear of the LeakyReLU kinks: no kink correction is needed.
    model(ps, (W, a, Wo)) -> a tuple that ends in the model's outputs.  -> ((W, a, Wo), *that tuple); the outputs gain "seed" = ps."""
    for ps in range(40):
        P = orc.xavier_params(cfg, ps)
        out = model(ps, P)
        if clear(out[-1]):
            out[-1]["seed"] = ps
            return (P, *out)
    raise AssertionError("no parameter seed clear of the LeakyReLU kink")


def run_model(cfg, g, P, **kw):
    return SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, **kw)


def pick_case(orc, cfg, g, mode, norm=False, reg=None, keeps=None, clear=None, **kw):
    """pick_params for a residual / norm case: mode (name, linear, bias) or None, Wres / b of xavier_wres(ps), gamma / beta of ln_params(ps)
    with norm, the masks of reg (keeps: given masks instead of reg's).  clear defaults to the bounds of the feature: CLEAR_V with the
    norm, else CLEAR_HPRE.  **kw goes to step_ref.forward.  -> (W, a, Wo), dict(Wres, b, gamma, beta: None where absent), outputs."""
    _, lin, bias = mode or (None, False, False)
    k, attn, feat = masks(cfg, g, cfg.heads, reg)
    keeps = k if keeps is None else keeps

    def model(ps, P):
        Wres, b = SR.xavier_wres(cfg, ps)            # b non-zero
        gamma, beta = SR.ln_params(cfg, ps) if norm else (None, None)
        inp = dict(Wres=Wres if lin else None, b=b if bias else None, gamma=gamma, beta=beta)
        return inp, run_model(cfg, g, P, **inp, eps=EPS, keeps=keeps, attn=attn, feat=feat, **kw)
    return pick_params(orc, cfg, model, clear or (CLEAR_V if norm else CLEAR_HPRE))


# -- a context against the model
def compare(pkg, ctx, g, cfg, ref, loss, tol, taps, groups):
    """loss / N at tol; every layer's tap named in taps ("hpre": GAT_TAP_HPRE, "hout": GAT_TAP_HOUT, "G": GAT_TAP_G = dL/dh_pre) and the
    gradient groups named in groups at tol of max-abs (recorded).  ref: the model's outputs after loss.backward(); a group the model
    does not have must be empty on the device."""
    A = pkg.abi
    n = g["n"]
    want_loss = ref["loss"].item()
    parity.record("loss/N", abs(loss / n - want_loss / n), tol, kind="abs")
    assert abs(loss / n - want_loss / n) < tol, (loss / n, want_loss / n)
    tap_of = {"hpre": (A.TAP_HPRE, lambda l: ref["hpre"][l]), "hout": (A.TAP_HOUT, lambda l: ref["hout"][l]),
              "G": (A.TAP_G, lambda l: ref["hpre"][l].grad)}
    for l in range(cfg.L):
        for name in taps:
            tap, want = tap_of[name]
            want = want(l).detach().numpy()
            assert np.abs(want).max() > 0
            parity.check_rel(f"{name}[{l}]", ctx.tap(tap, l).reshape(want.shape), want, tol)
    for name, got in zip(groups, grads(pkg, ctx, groups)):
        leaf = ref[name]
        if leaf is None:
            assert got.size == 0, name
            continue
        want = leaf.grad.numpy()
        assert got.shape == want.shape and np.abs(want).max() > 0
        parity.check_rel(f"grad {name}", got, want, tol)


def adam64(p, g, m, v, lr, b1, b2, eps, t):
    m[:] = b1 * m + (1.0 - b1) * g
    v[:] = b2 * v + (1.0 - b2) * g * g
    p -= lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps)


# -- shards
def shard_problem():
    return make_graph(4, n=90, e=700, F=12, C=4)


def shard_inputs(orc, g, norm):
    """The parameter groups of the shard tests, in the ABI's order: five with both residual flags, seven with the norm too."""
    cfg = orc.Config([8, 8], [8, 8], g["f"], g["c"])
    return (*orc.xavier_params(cfg, 11), *SR.xavier_wres(cfg, 11), *(SR.ln_params(cfg, 11) if norm else ()))


def shard_worker(rank, world, outdir, shm, replicate, norm):
    """One rank of a host-transport step on shard_problem with both residual flags (norm: and the layer norm): loss, correct and all
    the gradient groups go to outdir/r<rank>.npz."""
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as entry
    pkg = entry.load_package(); orc = entry.load_oracle()
    g = shard_problem()
    heads, outdims = [8, 8], [8, 8]
    S = pkg.shard
    plan = S.make_plan(g["row_ptr"], world, rank)
    rp_l, ci_l = S.local_csr(plan, g["row_ptr"], g["col_idx"])
    lo, hi = plan.row0, plan.row0 + plan.n_rows
    ctx = pkg.GatContext(heads, outdims, g["f"], g["c"], device=0)
    ctx.set_residual(linear=True, bias=True)
    if norm:
        ctx.set_norm(eps=EPS)
    ctx.set_graph(rp_l, ci_l, n_table=plan.n_table, table_row0=plan.table_row0)
    if replicate:
        ctx.set_source_features(plan.table_features(g["x"]))
    else:
        ctx.set_features(g["x"][lo:hi])
    ctx.set_labels(g["labels"][lo:hi])
    inputs = shard_inputs(orc, g, norm)
    for grp, arr in enumerate(inputs):
        ctx.params_set(grp, arr)
    ctx.comm_init_host(world, rank, shm, 4 * max(plan.n_table * 64, ctx.n_params + 3))
    ctx.zero_grad()
    loss, correct = ctx.step()
    grads = np.concatenate([ctx.grads_get(k) for k in range(len(inputs))])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), loss=loss, correct=correct, grads=grads)
    ctx.close()
