#!/usr/bin/env python3
"""dump_outputs.py GROUP OUT.npz — every output of the head for one group of cases, from the library GATV2_LIB names (unset: the tree's own),
as raw arrays for compare_outputs.py.  One process per (library, group, environment): run_outputs.sh chains them.

Groups: "head" = tests/head_cases.CASES; "child:<key>" = the cases of head_cases.CHILDREN[key] (the caller sets that key's environment);
"loss" = the (C, D_last, mode) sweep of tests/test_loss_modes.py at 129 and 300 rows, gat_step and gat_forward + gat_backward;
"kinds" = one readout, one pair and one hidden-head context in the softmax mode and in BCE.
Per case: y, loss, #correct, grad_Wo (every parameter group for "kinds"), the last layer's g tap, gat_eval_mask's result."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import head_cases as hc  # noqa: E402
import loss_ref as LR  # noqa: E402

pkg = entry.load_package()
A = pkg.abi
OUT = {}


def put(case, **arrays):
    for k, v in arrays.items():
        if v is not None:
            OUT[f"{case}/{k}"] = np.ascontiguousarray(v)


def scalars(loss, correct):
    return np.array([loss], np.float32), np.array([correct], np.int64)


def params(ctx, inp):
    for grp, k in ((A.PARAM_W, "W"), (A.PARAM_A, "a"), (A.PARAM_WO, "Wo")):
        ctx.params_set(grp, inp[k])


def head_case(case):
    """The run of head_cases.run_case without its reference."""
    inp = hc.make_inputs(case)
    L = len(case.heads) - 1
    with pkg.GatContext(case.heads, case.outdims, case.in_dim, case.C, keep_taps=case.keep_taps, flat_lrelu_index=case.flat,
                        dtype=case.dtype) as ctx:
        ctx.set_graph(inp["rp"], inp["ci"]); ctx.set_features(inp["x"]); ctx.set_labels(inp["lab"])
        params(ctx, inp)
        if case.wo in ("saturated", "tie"):
            ctx.forward(want_loss=False)
            hc.finish_inputs(case, inp, ctx.tap(A.TAP_HOUT, L))
            ctx.set_labels(inp["lab"]); ctx.params_set(A.PARAM_WO, inp["Wo"])
        if case.masked:
            ctx.set_train_mask(inp["mask"])
        ctx.zero_grad()
        if case.refused:
            loss, correct = ctx.forward()
        elif case.mode == "step":
            loss, correct = ctx.step()
        else:
            loss, correct = ctx.forward()
            ctx.backward()
        l, c = scalars(loss, correct)
        put(case.name, loss=l, correct=c, y=ctx.tap(A.TAP_Y), eval=np.array(ctx.eval_mask(inp["split"]), np.float64),
            gWo=None if case.refused else ctx.grads_get(A.PARAM_WO), g=None if case.refused else ctx.tap(A.TAP_G, L))


def loss_case(C, last, mode, n, how):
    """The run of test_loss_modes.run_head_case without its reference, with gat_eval_mask."""
    H, DL = last
    case = hc.Case(f"loss-{mode}-C{C}-h{H}d{DL}-n{n}", C, last, n=n, layers=1, in_dim=10)
    inp = hc.make_inputs(case)
    T = LR.targets_for(pkg, mode, n, C, seed=C * 1000 + n)
    with pkg.GatContext(case.heads, case.outdims, case.in_dim, C) as ctx:
        ctx.set_loss(mode)
        ctx.set_graph(inp["rp"], inp["ci"]); ctx.set_features(inp["x"]); ctx.set_targets(T)
        params(ctx, inp)
        ctx.set_train_mask(LR.row_mask(n, seed=n))
        ctx.zero_grad()
        if how == "step":
            loss, correct = ctx.step()
        else:
            loss, correct = ctx.forward()
            ctx.backward()
        l, c = scalars(loss, correct)
        put(f"{case.name}-{how}", loss=l, correct=c, y=ctx.tap(A.TAP_Y), gWo=ctx.grads_get(A.PARAM_WO), g=ctx.tap(A.TAP_G, 0),
            eval=np.array(ctx.eval_mask(inp["split"]), np.float64))


def kind_case(kind, mode):
    case = hc.Case(f"{kind}-{mode}", 47, (8, 8), n=300)
    inp = hc.make_inputs(case)
    rng = np.random.default_rng(7)
    with pkg.GatContext(case.heads, case.outdims, case.in_dim, case.C) as ctx:
        if kind == "hidden":
            ctx.set_head_hidden(32, "relu")
        if mode != "softmax":
            ctx.set_loss(mode)
        ctx.set_graph(inp["rp"], inp["ci"])
        rows = case.n
        if kind == "readout":
            ptr = np.array([0, 40, 41, 170, 300], np.int32)
            ctx.set_readout("mean", graph_ptr=ptr)
            rows = len(ptr) - 1
        if kind == "pair":
            rows = 333
            ctx.set_pairs("mul", rng.integers(0, case.n, rows).astype(np.int32), rng.integers(0, case.n, rows).astype(np.int32))
        ctx.set_features(inp["x"])
        if mode == "softmax":
            ctx.set_labels(rng.integers(0, case.C, rows).astype(np.int32))
        else:
            ctx.set_targets(LR.targets_for(pkg, mode, rows, case.C, seed=11))
        groups = A.PARAM_GROUPS_ALL if kind == "hidden" else A.PARAM_GROUPS
        for g in groups:
            cnt = ctx.param_count(g)
            if cnt:
                ctx.params_set(g, rng.uniform(-0.5, 0.5, cnt).astype(np.float32))
        for how in ("step", "fwdbwd"):
            ctx.zero_grad()
            if how == "step":
                loss, correct = ctx.step()
            else:
                loss, correct = ctx.forward()
                ctx.backward()
            l, c = scalars(loss, correct)
            put(f"{case.name}-{how}", loss=l, correct=c, y=ctx.tap(A.TAP_Y), eval=np.array(ctx.eval_mask(rng.random(rows) < 0.5), np.float64),
                **{f"grad{g}": ctx.grads_get(g) for g in groups if ctx.param_count(g)})


def main():
    group, out = sys.argv[1], sys.argv[2]
    if group == "head":
        for case in hc.CASES:
            head_case(case)
    elif group.startswith("child:"):
        for case in hc.CHILDREN[group[6:]][1]:
            head_case(case)
    elif group == "loss":
        import test_loss_modes as TL
        for C, last, mode in TL.HEAD_CASES:
            if C * last[1] <= 2048:
                for n in (129, 300):
                    for how in ("step", "fwdbwd"):
                        loss_case(C, last, mode, n, how)
    elif group == "kinds":
        for kind in ("readout", "pair", "hidden"):
            for mode in ("softmax", LR.BCE):
                kind_case(kind, mode)
    else:
        raise SystemExit(f"unknown group {group}")
    np.savez(out, **OUT)
    print(f"{group}: {len(OUT)} arrays from {os.environ.get('GATV2_LIB', 'the tree library')} switches {A.switches()!r}", flush=True)


if __name__ == "__main__":
    main()
