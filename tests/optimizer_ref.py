"""fp64 statement of the optimizer law of include/gatv2_abi.h ("optimizer step on the device").  The hyper-parameters arrive as the
float32 values the C ABI receives (f32()), everything else is float64.  One function for the clip factors, one per kind; `Model`
only strings them together over a packed buffer with its group slices, so that a test states a configuration once.

test_optimizer_fused_cpu.py holds these functions to torch (SGD, Adam, AdamW, clip_grad_norm_) at 1e-12; test_optimizer_fused.py holds
the kernels to them."""
import numpy as np

CLIP_NONE, CLIP_PER_GROUP, CLIP_GLOBAL = 0, 1, 2
SGD, ADAM, ADAMW = 1, 2, 3
EPS_GROUP = np.float64(np.float32(1e-9))           # the two guard constants are float32 literals in the kernels
EPS_GLOBAL = np.float64(np.float32(1e-6))


def f32(x):
    """A hyper-parameter as the ABI receives it."""
    return np.float64(np.float32(x))


def clip_factors(grads, mode, thr):
    """grads: the groups' gradients in ascending group order (empty groups allowed).  Returns (c [groups], group norms, global norm)."""
    s = [float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads]
    norms = np.sqrt(np.array(s, np.float64))
    total = float(np.sqrt(np.sum(s)))
    if mode == CLIP_NONE:
        return np.ones(len(grads)), norms, total
    thr = f32(thr)
    if mode == CLIP_PER_GROUP:
        c = np.array([thr / (n + EPS_GROUP) if n > thr else 1.0 for n in norms], np.float64)
        return c, norms, total
    if mode == CLIP_GLOBAL:
        q = thr / (total + EPS_GLOBAL)
        return np.full(len(grads), min(1.0, q) if q == q else q, np.float64), norms, total
    raise ValueError(mode)


def sgd(p, ghat, buf, lr, lam, mu, nesterov):
    """In place on p (and buf, which may be None when mu == 0).  lam: per entry (0 where the group's decay bit is clear)."""
    d = ghat + lam * p
    if mu > 0:
        buf[:] = mu * buf + d
        d = d + mu * buf if nesterov else buf
    p -= lr * d
    return d


def adam(p, ghat, m, v, lr, lam, b1, b2, eps, t):
    """Adam with L2 weight decay (torch.optim.Adam(weight_decay=)), in place."""
    d = ghat + lam * p
    m[:] = b1 * m + (1.0 - b1) * d
    v[:] = b2 * v + (1.0 - b2) * d * d
    p -= lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps)


def adamw(p, ghat, m, v, lr, lam, b1, b2, eps, t):
    """Decoupled weight decay (torch.optim.AdamW), in place."""
    p *= 1.0 - lr * lam
    m[:] = b1 * m + (1.0 - b1) * ghat
    v[:] = b2 * v + (1.0 - b2) * ghat * ghat
    p -= lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps)


class Model:
    """The configuration of gat_set_optimizer over a packed buffer: counts = the group sizes in ascending group order."""

    def __init__(self, counts, kind, lr, momentum=0.0, nesterov=False, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decay_groups=None,
                 clip_mode=CLIP_NONE, clip_threshold=0.0):
        self.counts = list(counts)
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.n = int(self.off[-1])
        self.kind, self.nesterov = kind, bool(nesterov)
        self.lr, self.mu, self.b1, self.b2, self.eps = f32(lr), f32(momentum), f32(betas[0]), f32(betas[1]), f32(eps)
        self.clip_mode, self.thr = clip_mode, clip_threshold
        groups = range(len(self.counts)) if decay_groups is None else decay_groups
        self.lam = np.zeros(self.n)
        for k in groups:
            self.lam[self.off[k]:self.off[k + 1]] = f32(weight_decay)
        self.t = 0
        self.m, self.v, self.buf = np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
        self.norms, self.global_norm = np.zeros(len(self.counts)), 0.0
        self.last = {}

    def split(self, flat):
        return [flat[self.off[k]:self.off[k + 1]] for k in range(len(self.counts))]

    def step(self, p, g):
        """One step in place on the float64 p, from the gradient g (float32 values, only read).  Leaves the step's magnitudes in
        self.last (|p| before, |ghat|, |buf| after) for the rounding bounds."""
        g = np.asarray(g, np.float64)
        c, self.norms, self.global_norm = clip_factors(self.split(g), self.clip_mode, self.thr)
        ghat = np.concatenate([ck * gk for ck, gk in zip(c, self.split(g))]) if self.n else g
        self.t += 1
        self.last = {"p": np.abs(p).copy(), "ghat": np.abs(ghat)}
        if self.kind == SGD:
            sgd(p, ghat, self.buf if self.mu > 0 else None, self.lr, self.lam, self.mu, self.nesterov)
        elif self.kind == ADAM:
            adam(p, ghat, self.m, self.v, self.lr, self.lam, self.b1, self.b2, self.eps, self.t)
        elif self.kind == ADAMW:
            adamw(p, ghat, self.m, self.v, self.lr, self.lam, self.b1, self.b2, self.eps, self.t)
        else:
            raise ValueError(self.kind)
        self.last["buf"] = np.abs(self.buf).copy()
        return p
