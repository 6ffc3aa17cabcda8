"""The heads of the fp64 step model (tests/step_ref.py::forward's head=): which rows the head reads, the optional hidden layer in front
of the output layer, and the three losses — each written once.
    rows    node: hout of the last layer;  readout: readout_ref.pool of it over graph_ptr;  pair_mul / pair_add: pair_ref.gather of it
    hidden  A = Xin W1^T,  Z1 = act(A + b1)                       (include/gatv2_abi.h "hidden layer")
    logits  z = Xin Wo^T  (Wo [C][D_last]),  or  z = Z1 Wo^T  (Wo [C][Dh])
    softmax y = exp(z - max) / (sum + 1e-8),  l = -log(max(y[label], 1e-12))
    BCE     y = sigmoid(z),  l = max(z,0) - t z + log1p(exp(-|z|))          MSE   y = z,  l = (z - t)^2
over the rows inside the mask and, for BCE / MSE, the target entries that are not NaN."""
import numpy as np

KINDS = ("node", "readout", "pair_mul", "pair_add")
SOFTMAX, BCE, MSE = "softmax", "bce", "mse"
SLOPE = 0.01                      # GatContext's default negative_slope (the lrelu activation's)


def act(t, name):
    """torch: ReLU, or LeakyReLU with SLOPE; at exactly 0 the derivative is the slope branch's (torch's convention for both)."""
    import torch
    return torch.relu(t) if name == "relu" else torch.nn.functional.leaky_relu(t, SLOPE)


def contributes(T, mask=None):
    """[R][C] bool: the entry is present (not NaN) and its row trains."""
    T = np.asarray(T)
    rows = np.ones(T.shape[0], bool) if mask is None else np.asarray(mask) != 0
    return ~np.isnan(T) & rows[:, None]


def head_input(out, kind, graph_ptr=None, u=None, v=None, pool_mode="mean"):
    """The rows the head reads, attached to the autograd graph of the model's dict `out`."""
    import pair_ref
    import readout_ref
    X = out["hout"][-1]
    if kind == "node":
        return X
    if kind == "readout":
        return readout_ref.pool(X, graph_ptr, pool_mode)[0]
    return pair_ref.gather(X, u, v, "mul" if kind == "pair_mul" else "add")


def hidden(xin, W1, b1, act_name):
    """W1 flat [Dh][D_in], b1 [Dh] (torch) -> (A = Xin W1^T, the activation's argument A + b1, Z1)."""
    A = xin @ W1.view(b1.shape[0], -1).t()
    pre = A + b1
    return A, pre, act(pre, act_name)


def loss(z, kind, sup, mask=None, detach_max=True, smooth_bce=False):
    """The loss `kind` on the logits z [R][C] (torch fp64): SOFTMAX with sup = labels [R], BCE / MSE with sup = targets [R][C] (NaN =
    missing); mask [R] or None: rows outside it send no loss.  -> (loss sum, y, the loss per row or None for BCE / MSE), torch, attached.
    detach_max: the softmax's row maximum is a constant to autograd, as the kernels' is.  False keeps it attached: with the 1e-8 guard y
        depends on the maximum (by 1e-8 of itself), and a detached one leaves autograd that far from the function's derivative —
        nothing at the 1e-4 bars, but visible to central differences at 1e-8.
    smooth_bce: torch's binary_cross_entropy_with_logits instead of the max form above.  The max form has the autograd subgradient
        1 - t at z == 0 exactly, where the derivative is sigmoid(0) - t = 0.5 - t (the header's dz = y - t).  A head row of exact zeros —
        MUL pairs with an endpoint whose row is 0, as the graph's empty row is — has z == 0, and its gradient reaches the G taps."""
    import torch
    if kind == SOFTMAX:
        m = z.max(dim=1, keepdim=True).values
        ez = torch.exp(z - (m.detach() if detach_max else m))
        y = ez / (ez.sum(1, keepdim=True) + 1e-8)
        lab = torch.from_numpy(np.asarray(sup)).long()
        per = -torch.log(torch.clamp(y[torch.arange(z.shape[0]), lab], min=1e-12))
        if mask is None:
            return per.sum(), y, per
        return (per * torch.from_numpy(np.asarray(mask, bool).astype(np.float64))).sum(), y, per
    on = contributes(sup, mask)
    t = torch.from_numpy(np.where(on, np.nan_to_num(np.asarray(sup, np.float64)), 0.0))
    if kind == MSE:
        per, y = (z - t) ** 2, z
    else:
        y = torch.sigmoid(z)
        if smooth_bce:
            per = torch.nn.functional.binary_cross_entropy_with_logits(z, t, reduction="none")
        else:
            per = torch.clamp(z, min=0) - t * z + torch.log1p(torch.exp(-z.abs()))
    return (per * torch.from_numpy(on.astype(np.float64))).sum(), y, None


def head(kind, loss_kind, sup, mask=None, graph_ptr=None, u=None, v=None, pool_mode="mean", Wo=None, W1=None, b1=None, act_name="relu",
         detach_max=True, smooth_bce=False):
    """-> step_ref.forward's head=: head_input, the hidden layer where W1 / b1 are given, the logits and loss().  Wo None: the model's
    own leaf out["Wo"]; Wo / W1 / b1 given here become leaves rounded to fp32, flat as the ABI's groups, and join the dict.  The dict
    also gains xin (the head's rows, grad retained), z and y (numpy), loss_per_row (numpy; None for BCE / MSE) and, with the hidden
    layer, A and pre (numpy) and z1 (grad retained)."""
    import torch
    leaf = lambda a_: torch.from_numpy(np.asarray(a_, np.float32).astype(np.float64).reshape(-1)).requires_grad_(True)

    def run(out):
        xin = rows = head_input(out, kind, graph_ptr, u, v, pool_mode)
        if xin.requires_grad:
            xin.retain_grad()
        if Wo is not None:
            out["Wo"] = leaf(Wo)
        if W1 is not None:
            out["W1"], out["b1"] = leaf(W1), leaf(b1)
            A, pre, rows = hidden(xin, out["W1"], out["b1"], act_name)
            rows.retain_grad()
            out.update(A=A.detach().numpy(), pre=pre.detach().numpy(), z1=rows)
        z = rows @ out["Wo"].view(-1, rows.shape[1]).t()
        total, y, per = loss(z, loss_kind, sup, mask, detach_max, smooth_bce)
        out.update(xin=xin, z=z.detach().numpy(), y=y.detach().numpy(), loss_per_row=None if per is None else per.detach().numpy())
        return total
    return run
