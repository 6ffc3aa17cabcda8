"""Plain fp64 numpy reference of the output head (TEST INFRASTRUCTURE): logits, softmax, loss, prediction and the
head's backward, with the library's contract (include/gatv2_abi.h; E:463-608):

    z = H_L · Woᵀ                        y = exp(z - max) / (sum + 1e-8)
    nll = -log(max(float32(y[label]), 1e-12))          pred = first maximum of y
    dz = y - onehot (0 outside the training mask)      gH = dz · Wo        gradWo = dzᵀ · H_L
    g[n, h, d] = gH[n, d] · LReLU'(h_pre[n, h, d]) / H            (flat_index: h_pre.reshape(-1)[n·D_last + d], E:598)

Everything is evaluated in float64 from the inputs as given; the only float32 step is the cast of y[label] in front
of the clamp, which is where the contract puts it (the probabilities are stored as float32).

`undecided`: nodes whose two largest probabilities differ by less than UNDECIDED_REL of the larger one — an fp32
evaluation may order them either way — EXCEPT where the Wo rows of all classes that close to the top are bit-identical:
those logits are equal in any arithmetic that treats equal operands equally, the tie is exact, and the first wins.
"""
from typing import NamedTuple

import numpy as np

UNDECIDED_REL = 1e-5
CLAMP = 1e-12


class HeadRef(NamedTuple):
    y: np.ndarray          # [N][C] float64
    nll: np.ndarray        # [N] float64, every node (the training loss is nll[mask].sum())
    pred: np.ndarray       # [N] int64, first maximum
    dz: np.ndarray         # [N][C]
    gH: np.ndarray         # [N][D_last]
    gradWo: np.ndarray     # [C][D_last]
    g: np.ndarray          # [N][H][D_last]
    undecided: np.ndarray  # sorted node ids


def logits(HL, Wo):
    HL = np.asarray(HL, np.float64)
    return HL @ np.asarray(Wo, np.float64).reshape(-1, HL.shape[1]).T


def head_ref(HL, hpre, Wo, labels, mask, H, slope, flat_index=False) -> HeadRef:
    HL = np.asarray(HL, np.float64)
    N, DL = HL.shape
    Wo32 = np.ascontiguousarray(np.asarray(Wo, np.float32).reshape(-1, DL))
    Wo64 = Wo32.astype(np.float64)
    C = Wo64.shape[0]
    labels = np.asarray(labels, np.int64)
    mask = np.ones(N, bool) if mask is None else np.asarray(mask) != 0
    rows = np.arange(N)

    z = HL @ Wo64.T
    ez = np.exp(z - z.max(axis=1, keepdims=True))
    y = ez / (ez.sum(axis=1, keepdims=True) + 1e-8)
    plab = y[rows, labels].astype(np.float32).astype(np.float64)
    nll = -np.log(np.maximum(plab, CLAMP))
    pred = y.argmax(axis=1)                                   # numpy: the first of equal maxima

    # undecided nodes
    top = y.max(axis=1, keepdims=True)
    near = y > top * (1.0 - UNDECIDED_REL)                    # classes within the margin of the top (the top itself included)
    undecided = []
    for n in np.nonzero(near.sum(axis=1) > 1)[0]:
        cls = np.nonzero(near[n])[0]
        same = all(Wo32[c].tobytes() == Wo32[cls[0]].tobytes() for c in cls[1:])
        if same:
            pred[n] = cls[0]                                  # exact tie: identical rows give identical logits, first wins
        else:
            undecided.append(n)

    dz = y.copy()
    dz[rows, labels] -= 1.0
    dz[~mask] = 0.0
    gH = dz @ Wo64
    gradWo = dz.T @ HL
    hp = np.asarray(hpre, np.float64).reshape(N, H, DL)
    if flat_index:
        hp = np.broadcast_to(hp.reshape(-1)[:N * DL].reshape(N, 1, DL), (N, H, DL))
    g = gH[:, None, :] * np.where(hp > 0, 1.0, float(slope)) / float(H)
    return HeadRef(y, nll, pred, dz, gH, gradWo, g, np.asarray(undecided, np.int64))


def logit_rounding_bound(HL, Wo):
    """B of the saturated-softmax cases: mean over nodes of 2 (D_last + 1) 2⁻²⁴ max_c Σ_j |Wo[c,j]| |H_L[n,j]| — the
    fp32 rounding of the logits themselves (D_last products and sums at unit round-off 2⁻²⁴, once for the label's logit
    and once for the maximum the loss is measured from)."""
    HL = np.abs(np.asarray(HL, np.float64))
    DL = HL.shape[1]
    aw = np.abs(np.asarray(Wo, np.float64).reshape(-1, DL))
    return float((2.0 * (DL + 1) * 2.0 ** -24 * (HL @ aw.T).max(axis=1)).mean())
