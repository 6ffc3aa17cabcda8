"""What the batch-normalisation tests share (tests/test_batchnorm.py, test_batchnorm_kernels.py, test_batchnorm_cpu.py): the context
builder (feature_cases.make_ctx with gat_set_batch_norm in gat_set_norm's place), the seed search against the fp64 model of
tests/step_ref.py (bn=True), the comparison of the four statistics vectors, and the table of the kernel tests with its fp64 numpy model.  A
plain module: the test modules import it, never each other."""
import numpy as np

import batchnorm_ref as BR
import feature_cases as FC
import head_model as HD
import parity
import step_ref as SR

EPS = FC.EPS
MOMENTUM = 0.1
MODES = [("bn", False, False), ("bn_res", True, True)]          # (name, GAT_RES_LINEAR, GAT_RES_BIAS)
GROUPS = FC.GROUPS[:7]
TAPS = ["hpre", "hout", "G"]
STATS = ("running_mean", "running_var", "batch_mean", "batch_rstd")     # GAT_BN_RUNNING_MEAN .. GAT_BN_BATCH_RSTD


def make_ctx(pkg, g, heads, outdims, P, *, Wres=None, b=None, gamma=None, beta=None, residual=None, bn=None, reg=None, **kw):
    """feature_cases.make_ctx for a batch-norm context.  bn: keyword arguments of set_batch_norm ({}: its defaults but eps = EPS; None: the
    call is not made)."""
    ctx = pkg.GatContext(heads, outdims, g["f"], g["c"], **kw)
    if bn is not None:
        ctx.set_batch_norm(**dict(dict(eps=EPS, momentum=MOMENTUM), **bn))
    if residual is not None:
        ctx.set_residual(linear=residual[0], bias=residual[1])
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


def setters(mode, skip_last=False):
    return dict(residual=mode[1:] if mode[1] or mode[2] else None, bn=dict(skip_last=skip_last))


def run_model(cfg, g, P, bn=True, **kw):
    return SR.forward(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P, bn=bn, **kw)


SEEDS = 400


def pick_params(orc, cfg, model, clear):
    """feature_cases.pick_params over SEEDS seeds instead of 40: a column statistic couples every row of a column, and the seeds that keep
    every non-zero |s| above 1e-5 AND every |v| above 1e-4 are a few in a hundred here (one model run takes some 30 ms)."""
    for ps in range(SEEDS):
        P = orc.xavier_params(cfg, ps)
        out = model(ps, P)
        if clear(out[-1]):
            out[-1]["seed"] = ps
            return (P, *out)
    raise AssertionError("no parameter seed clear of the LeakyReLU kink")


def pick_case(orc, cfg, g, mode, reg=None, clear=None, **kw):
    """feature_cases.pick_case against the batch-norm model: Wres / b of xavier_wres(ps) where the mode has them, gamma / beta of
    ln_params(ps); seeds keep every non-zero |s| above 1e-5 and |v| above 1e-4 (FC.CLEAR_V, the layer norm's bound).  **kw goes to
    step_ref.forward.  -> (W, a, Wo), dict(Wres, b, gamma, beta), outputs."""
    _, lin, bias = mode
    keeps, attn, feat = FC.masks(cfg, g, cfg.heads, reg)

    def model(ps, P):
        Wres, b = SR.xavier_wres(cfg, ps)
        gamma, beta = SR.ln_params(cfg, ps)
        inp = dict(Wres=Wres if lin else None, b=b if bias else None, gamma=gamma, beta=beta)
        return inp, run_model(cfg, g, P, **inp, eps=EPS, keeps=keeps, attn=attn, feat=feat, momentum=MOMENTUM, **kw)
    return pick_params(orc, cfg, model, clear or FC.CLEAR_V)


def compare(pkg, ctx, g, cfg, ref, loss, tol, taps=TAPS):
    """feature_cases.compare for a batch-norm context: loss, the taps, all seven gradient groups.  grad_b of a batch-normalised layer is
    sum_n G[n,c], identically 0 (G has no column mean: the normalisation removes what a bias adds), and the model returns its own
    rounding, 1e-16, for it.  A sum that vanishes cannot be held to a fraction of its result; it is held to the same fraction of its
    terms' size, max_c sum_n |G[n,c]| — unless the model's group has a layer that is not normalised (skip_last), whose entries give the
    group a size of its own: then the bar is feature_cases.compare's."""
    FC.compare(pkg, ctx, g, cfg, ref, loss, tol, taps, [k for k in GROUPS if k != "b"])
    got = FC.grads(pkg, ctx, ["b"])[0]
    if ref["b"] is None:
        assert got.size == 0
        return
    want = ref["b"].grad.numpy()
    terms = max(float(ref["hpre"][l].grad.abs().reshape(ref["hpre"][l].shape[0], -1).sum(0).max()) for l in range(cfg.L))
    vanishing = float(np.abs(want).max()) <= 1e-9 * terms
    assert got.shape == want.shape
    parity.check_rel("grad b", got, want, tol, floor=terms if vanishing else 1e-12, vanishing=vanishing)


def compare_stats(pkg, ctx, ref, tol, which=STATS):
    """The statistics vectors of the context against the model's, at tol of max-abs (recorded)."""
    for i, name in enumerate(STATS):
        if name not in which:
            continue
        want = ref[name]
        assert np.abs(want).max() > 0
        parity.check_rel(name, ctx.batch_norm_stats(i), want, tol)


def all_stats(ctx):
    return [ctx.batch_norm_stats(i) for i in range(4)]


# -- the kernel tests (tests/test_batchnorm_kernels.py): shapes, inputs, the fp64 numpy model of the two seams
ROWS = (1, 2, 63, 64, 65, 1500)
SHAPES = ((1, 1), (1, 7), (8, 8), (2, 4), (5, 13), (20, 13), (3, 87))
SLOPE = 0.01
KERNEL_TOL = 1e-5           # of max-abs: fp32 sums of at most 1500 terms
KINK = 1e-4                 # |v| below this: the entry's output gradient is zeroed (kernel_inputs)


def kernel_inputs(n, H, D, seed=0):
    """u with a column offset and spread of its own per column (so a wrong column index shows), dL/dhout for both layer kinds, gamma
    U[0.5, 1.5], beta U[-0.5, 0.5], R, b, running statistics away from 0 / 1.  Where |v| < KINK of either mode the output gradient is 0
    (for the last layer: that (row, d) of gh), so that no result depends on the side of the LeakyReLU kink fp32 puts such an entry on.
    n == 2: the two rows of a column are sqrt(eps) * O(1) apart and centred on 0.  Two rows normalise to +-sqrt(var / (var + eps))
    whatever they hold, and the training-mode gradient is G = gamma (dv0 - dv1) / 2 * eps / (var + eps)^1.5: with var >> eps it is the
    1e-5 fraction its terms leave after cancelling, where nothing can be held to 1e-5 (the fp32 rounding of rstd alone moves it by a
    percent) and nothing is tested; with var ~ eps every term of the formula, eps included, carries weight."""
    rng = np.random.default_rng(1000 * n + 17 * H + D + seed)
    HD = H * D
    u = (rng.standard_normal((n, HD)) * rng.uniform(0.5, 2.0, HD) + rng.uniform(-1, 1, HD)).astype(np.float32)
    if n == 2:
        u = (np.sqrt(EPS) * rng.standard_normal((n, HD)) * rng.uniform(0.5, 2.0, HD)).astype(np.float32)
    inp = dict(u=u, g=rng.standard_normal((n, HD)).astype(np.float32), gh=rng.standard_normal((n, D)).astype(np.float32),
               gamma=rng.uniform(0.5, 1.5, HD).astype(np.float32), beta=rng.uniform(-0.5, 0.5, HD).astype(np.float32),
               res=rng.standard_normal((n, HD)).astype(np.float32), bias=rng.uniform(-0.5, 0.5, HD).astype(np.float32),
               run_mean=rng.uniform(-0.5, 0.5, HD).astype(np.float32), run_var=rng.uniform(0.5, 2.0, HD).astype(np.float32))
    near = np.zeros((n, HD), bool)
    for training in (True, False):
        near |= np.abs(kernel_model(inp, H, D, False, training)["v"]) < KINK
    inp["g"][near] = 0.0
    inp["gh"][near.reshape(n, H, D).any(1)] = 0.0
    return inp


def kernel_model(inp, H, D, is_last, training, eps=EPS, momentum=MOMENTUM, slope=SLOPE):
    """fp64 numpy model of gat_op_batch_norm_forward + _backward on kernel_inputs."""
    f8 = lambda k: inp[k].astype(np.float64)
    u, gamma, beta = f8("u"), f8("gamma"), f8("beta")
    n = u.shape[0]
    out = {}
    if training:
        mu = u.mean(0)
        var = ((u - mu) ** 2).mean(0)
        out["mean"], out["rstd"] = mu, 1.0 / np.sqrt(var + eps)
        out["run_mean"], out["run_var"] = BR.running_update(f8("run_mean"), f8("run_var"), mu, var, n, momentum)
    else:
        out["mean"], out["rstd"] = f8("run_mean"), 1.0 / np.sqrt(f8("run_var") + eps)
        out["run_mean"], out["run_var"] = f8("run_mean"), f8("run_var")
    xh = (u - out["mean"]) * out["rstd"]
    v = gamma * xh + beta
    act = np.where(v > 0, v, slope * v)
    out["v"] = v
    out["hout"] = act.reshape(n, H, D).mean(1) if is_last else act
    go = np.tile(f8("gh"), (1, H)) / H if is_last else f8("g")
    dv = go * np.where(v > 0, 1.0, slope)
    s1, s2 = dv.sum(0), (dv * xh).sum(0)
    if training:
        G = gamma * out["rstd"] * (dv - s1 / n - xh * s2 / n)
    else:
        G = gamma * out["rstd"] * dv
    out.update(grad_beta=s1, grad_gamma=s2, G=G, agg=u - (f8("res") + f8("bias")), grad_b=G.sum(0))
    return out


PROFILES = {"cap1": {"GAT_RESIDENT_CAP": "1"}, "cap3": {"GAT_RESIDENT_CAP": "3"}}     # as tests/trip_cases.py: one process per profile
KERNEL_CASES = [(n, H, D, is_last, training) for n in ROWS for (H, D) in SHAPES for is_last in (False, True) for training in (True, False)]
VECTORS = ("mean", "rstd", "run_mean", "run_var", "grad_gamma", "grad_beta", "grad_b")     # what a grid's summation order can change


def kernel_case_id(case):
    n, H, D, is_last, training = case
    return f"n{n}_h{H}_d{D}_{'last' if is_last else 'hidden'}_{'train' if training else 'eval'}"


def run_kernel_case(pkg, case, base=0.25):
    """One case through the two seams -> dict of numpy outputs (hout, mean, rstd, run_mean, run_var, G, agg, grad_gamma, grad_beta, grad_b).
    The three gradient vectors start at `base`: the seams ADD into them (returned with the base taken off again)."""
    import torch
    A = pkg.abi
    n, H, D, is_last, training = case
    HD = H * D
    inp = kernel_inputs(n, H, D)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(v) for k, v in inp.items()}
    mr = torch.full((2, HD), 7.0, device="cuda")         # (eval mode leaves it alone)
    hout = torch.empty((n, D if is_last else HD), device="cuda")
    G = torch.empty((n, HD), device="cuda"); agg = torch.empty((n, HD), device="cuda")
    gg, gb, gbias = (torch.full((HD,), base, device="cuda") for _ in range(3))
    p = lambda t: t.data_ptr()
    A.op_batch_norm_forward(p(d["u"]), n, H, D, is_last, p(d["gamma"]), p(d["beta"]), EPS, SLOPE, MOMENTUM, p(d["run_mean"]), p(d["run_var"]),
                            training, p(mr), p(hout))
    if training:
        rm, rv = p(d["run_mean"]), p(d["run_var"])       # the backward of training mode does not read them
    else:
        assert (mr == 7.0).all()
        rm, rv = p(d["run_mean"]), p(d["run_var"])
    A.op_batch_norm_backward(p(d["u"]), 0 if is_last else p(d["g"]), p(d["gh"]) if is_last else 0, D, n, H, D, p(d["gamma"]), p(d["beta"]),
                             p(mr), rm, rv, EPS, SLOPE, training, p(d["res"]), p(d["bias"]), p(G), p(agg), p(gg), p(gb), p(gbias))
    torch.cuda.synchronize()
    out = dict(hout=hout, G=G, agg=agg, run_mean=d["run_mean"], run_var=d["run_var"], grad_gamma=gg - base, grad_beta=gb - base, grad_b=gbias - base)
    if training:
        out.update(mean=mr[0], rstd=mr[1])
    return {k: v.cpu().numpy() for k, v in out.items()}


def kernel_scales(case, want):
    """What KERNEL_TOL is a fraction of, per output: the output's max-abs, but
    - the three vectors the seams ADD into (onto `base` = 0.25, taken off again): at least 2^-22 / KERNEL_TOL — "base + sum - base" keeps
      half an ulp of max(base, |sum|) twice;
    - grad_b in training mode: sum_n G[n,c] is identically 0 through the normalisation (G has no column mean), so its max-abs is the
      model's own rounding; what a float sum of N terms can be held to is a fraction of the terms' size: max_c sum_n |G[n,c]|."""
    training = case[4]
    out = {}
    for k, w in want.items():
        scale = float(np.abs(w).max()) if np.size(w) else 0.0
        if k.startswith("grad_"):
            scale = max(scale, 2.0 ** -22 / KERNEL_TOL)
        if k == "grad_b" and training:
            scale = max(scale, float(np.abs(want["G"]).sum(0).max()))
        out[k] = max(scale, 1e-12)
    return out


def check_kernel_case(pkg, case, outs=None):
    """run_kernel_case against kernel_model at KERNEL_TOL of kernel_scales, every output (recorded).  -> the outputs."""
    n, H, D, is_last, training = case
    got = run_kernel_case(pkg, case) if outs is None else outs
    want = kernel_model(kernel_inputs(n, H, D), H, D, is_last, training)
    scales = kernel_scales(case, want)
    cid = kernel_case_id(case)
    for k, v in got.items():
        parity.check_rel(f"{cid} {k}", v.reshape(want[k].shape), want[k], KERNEL_TOL, floor=scales[k])
    return got


def run_kernel_profile(pkg, outdir=None):
    """The whole table twice in this process: every case against the model, the two runs bitwise equal; the VECTORS of every case to
    outdir/vectors.npz.  -> (cases, failures)."""
    failures, saved = [], {}
    for case in KERNEL_CASES:
        cid = kernel_case_id(case)
        try:
            a = check_kernel_case(pkg, case)
            b = run_kernel_case(pkg, case)
            for k in a:
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (k, "two runs differ")
            scales = kernel_scales(case, kernel_model(kernel_inputs(*case[:3]), *case[1:]))
            for k in VECTORS:
                if k in a:
                    saved[f"{cid} {k}"] = a[k]
                    saved[f"{cid} {k} scale"] = np.float64(scales[k])
        except AssertionError as e:
            failures.append(cid)
            print("FAILED", cid, str(e)[:300])
    if outdir is not None:
        np.savez(f"{outdir}/vectors.npz", **saved)
    return len(KERNEL_CASES), failures


# -- one case per head kind (tests/test_batchnorm.py), against step_ref.forward(bn=True) with head_model.head
FE = 3
HEAD_CASES = {                                   # name -> (kind, loss, training mask, hidden width, edge features)
    "readout_mean": ("readout", "softmax", False, 0, False),
    "pair_mul_bce": ("pair_mul", "bce", False, 0, False),
    "hidden_head": ("node", "softmax", False, 16, False),
    "bce_mask": ("node", "bce", True, 0, False),
    "mse_mask": ("node", "mse", True, 0, False),
    "edge_features": ("node", "softmax", False, 0, True),
}


def head_case(pkg, orc, name):
    """Everything a head case runs on: records_d8 on parity_graph, BN + both residual flags, the supervision of tests/head_mlp_ref.py's
    cases, a seed clear of the kinks (|s| > 1e-5, |v| > 1e-4, the hidden stage's |A + b1| > A_MIN, softmax rows off the loss clamp)."""
    import edge_feat_ref as EF
    import head_mlp_ref as HM
    import loss_ref as LR
    import pair_ref as PR
    kind, loss, masked, dh, fe = HEAD_CASES[name]
    g = FC.parity_graph()
    if loss == "bce":
        g = dict(g, c=1, labels=np.zeros(g["n"], np.int32))
    heads, outdims = [8, 8], [8, 8]
    cfg = orc.Config(heads, outdims, g["f"], g["c"])
    graph_ptr = HM.GRAPH_PTR if kind == "readout" else None
    u, v = PR.pair_list(g["n"]) if kind.startswith("pair") else (None, None)
    R = len(u) if u is not None else len(graph_ptr) - 1 if graph_ptr is not None else g["n"]
    if loss == "softmax":
        sup = g["labels"] if kind == "node" else PR.pair_labels(R, g["c"])
    elif loss == "bce":
        sup = (np.random.default_rng(41).random((R, 1)) > 0.5).astype(np.float32)
    else:
        sup = LR.targets_for(pkg, "mse", R, g["c"])
    mask = LR.row_mask(R) if masked else None
    W1, b1, Wo_h = HM.head_values(outdims[-1], dh, g["c"]) if dh else (None, None, None)
    ea = EF.edge_attrs(g, FE) if fe else None

    def model(ps, P, **kw):
        Wres, b = SR.xavier_wres(cfg, ps)
        gamma, beta = SR.ln_params(cfg, ps)
        inp = dict(Wres=Wres, b=b, gamma=gamma, beta=beta)
        if fe:
            inp.update(ea=ea, We=SR.xavier_we(cfg, FE, ps))
        head = HD.head(kind, loss, sup, mask, graph_ptr=graph_ptr, u=u, v=v, Wo=Wo_h if dh else P[2], W1=W1, b1=b1, detach_max=False,
                       smooth_bce=True)
        return inp, run_model(cfg, g, P, **inp, eps=EPS, momentum=MOMENTUM, head=head, **kw)

    def clear(r):
        if not FC.CLEAR_V(r) or (dh and not float(np.abs(r["pre"]).min()) > HM.A_MIN):
            return False
        if loss != "softmax":
            return True
        keep = np.ones(R, bool) if mask is None else np.asarray(mask, bool)
        return float(r["y"][np.arange(R), np.asarray(sup)][keep].min()) > HM.Y_MIN
    P, inp, ref = pick_params(orc, cfg, model, clear)
    return dict(g=g, heads=heads, outdims=outdims, cfg=cfg, P=P, inp=inp, ref=ref, kind=kind, loss=loss, sup=sup, mask=mask, dh=dh, W1=W1, b1=b1,
                Wo=Wo_h if dh else P[2], graph_ptr=graph_ptr, u=u, v=v, rows=R)


def make_head_ctx(pkg, ci, **kw):
    """The context of a head case (the order of calls of tests/head_mlp_ref.make_ctx), parameters set, gradients zeroed."""
    A = pkg.abi
    g, inp, kind = ci["g"], ci["inp"], ci["kind"]
    ctx = pkg.GatContext(ci["heads"], ci["outdims"], g["f"], g["c"], **kw)
    ctx.set_batch_norm(eps=EPS, momentum=MOMENTUM)
    if inp.get("We") is not None:
        ctx.set_edge_dim(FE)
    ctx.set_residual(linear=True, bias=True)
    if ci["loss"] != "softmax":
        ctx.set_loss(ci["loss"])
    if ci["dh"]:
        ctx.set_head_hidden(ci["dh"], "relu")
    ctx.set_graph(g["row_ptr"], g["col_idx"])
    ctx.set_features(g["x"])
    if kind == "readout":
        ctx.set_readout("mean", graph_ptr=ci["graph_ptr"])
    elif kind.startswith("pair"):
        ctx.set_pairs("mul" if kind == "pair_mul" else "add", ci["u"], ci["v"])
    if ci["loss"] == "softmax":
        ctx.set_labels(ci["sup"])
    else:
        ctx.set_targets(ci["sup"])
    if inp.get("ea") is not None:
        ctx.set_edge_features(inp["ea"])
    for grp, name in ((A.PARAM_WRES, "Wres"), (A.PARAM_B, "b"), (A.PARAM_NORM_G, "gamma"), (A.PARAM_NORM_B, "beta"), (A.PARAM_WE, "We")):
        if inp.get(name) is not None:
            ctx.params_set(grp, inp[name])
    ctx.params_set(A.PARAM_W, ci["P"][0]); ctx.params_set(A.PARAM_A, ci["P"][1]); ctx.params_set(A.PARAM_WO, ci["Wo"])
    if ci["dh"]:
        ctx.params_set(A.PARAM_HEAD_W, ci["W1"]); ctx.params_set(A.PARAM_HEAD_B, ci["b1"])
    if ci["mask"] is not None:
        ctx.set_train_mask(ci["mask"])
    ctx.zero_grad()
    return ctx
