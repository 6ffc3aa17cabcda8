"""CPU self-test of tests/head_ref.py (the fp64 reference the GPU head tests compare with): its gradients against torch
fp64 autograd of the same loss, its loss against torch's cross-entropy, and its tie / undecided rules."""
import numpy as np
import pytest
import torch

import head_ref as hr

SLOPE = 0.01
SHAPES = [  # N, C, H, D_last, masked
    (37, 7, 8, 8, False),
    (64, 47, 1, 12, True),
    (5, 300, 8, 4, False),
]


def _inputs(n, c, h, d, masked, seed):
    rng = np.random.default_rng(seed)
    HL = rng.standard_normal((n, d)).astype(np.float32)
    hpre = rng.standard_normal((n, h, d)).astype(np.float32)
    Wo = (rng.standard_normal((c, d)) * 0.7).astype(np.float32)
    lab = rng.integers(0, c, n).astype(np.int32)
    mask = np.ones(n, bool)
    if masked:
        mask = rng.random(n) > 0.4
        mask[0] = mask[-1] = False
    return HL, hpre, Wo, lab, mask


@pytest.mark.parametrize("n,c,h,d,masked", SHAPES)
def test_against_autograd(n, c, h, d, masked):
    HL, hpre, Wo, lab, mask = _inputs(n, c, h, d, masked, 100 + c)
    ref = hr.head_ref(HL, hpre, Wo, lab, mask, h, SLOPE, False)
    tH = torch.tensor(HL, dtype=torch.float64, requires_grad=True)
    tW = torch.tensor(Wo, dtype=torch.float64, requires_grad=True)
    z = tH @ tW.T
    ez = torch.exp(z - z.max(dim=1, keepdim=True).values.detach())        # the shift is a constant of the contract, not a variable
    y = ez / (ez.sum(dim=1, keepdim=True) + 1e-8)
    tl = torch.tensor(lab, dtype=torch.int64)
    nll = -torch.log(y[torch.arange(n), tl])
    nll[torch.tensor(mask)].sum().backward()

    def rel(a, b):
        return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))
    assert rel(ref.y, y.detach().numpy()) <= 1e-12
    assert rel(ref.gradWo, tW.grad.numpy()) <= 1e-12
    assert rel(ref.gH, tH.grad.numpy()) <= 1e-12
    # the loss: float32(y[label]) in front of the log costs half an ulp of fp32; the 1e-8 in the denominator 1e-8
    ce = torch.nn.functional.cross_entropy(z.detach(), tl, reduction="none").numpy()
    assert np.abs(ref.nll - ce).max() <= 1e-7
    assert np.array_equal(ref.pred, z.detach().numpy().argmax(1)) and ref.undecided.size == 0
    # g, entry by entry, both index modes
    for flat in (False, True):
        g = hr.head_ref(HL, hpre, Wo, lab, mask, h, SLOPE, flat).g
        flat_hp = hpre.reshape(-1)
        for nn in (0, n // 2, n - 1):
            for hh in range(h):
                for dd in range(d):
                    hp = flat_hp[nn * d + dd] if flat else hpre[nn, hh, dd]
                    want = ref.gH[nn, dd] * (1.0 if hp > 0 else SLOPE) / h
                    assert g[nn, hh, dd] == pytest.approx(want, rel=1e-15, abs=0)
    if masked:
        assert not ref.dz[~mask].any() and not ref.g[~mask].any()


def test_clamp_ties_and_undecided():
    HL = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], np.float32)
    hpre = np.ones((3, 1, 2), np.float32)
    # node 0: class 1 and 3 have bit-identical rows and lead -> exact tie, the first (1) wins, decided
    # node 1: classes 0 and 2 differ in the last bit of a weight -> within the margin, different rows: undecided
    # node 2: class 1/3 lead clearly
    w = np.float32(3.0)
    Wo = np.array([[0.0, w], [5.0, 0.0], [0.0, np.nextafter(w, np.float32(4))], [5.0, 0.0]], np.float32)
    ref = hr.head_ref(HL, hpre, Wo, [3, 0, 1], None, 1, SLOPE)
    assert ref.pred[0] == 1 and ref.pred[2] == 1
    assert ref.undecided.tolist() == [1]
    # saturation: the label's probability underflows float32 -> the clamp, exactly
    ref = hr.head_ref(HL * 200, hpre, Wo, [0, 1, 0], None, 1, SLOPE)
    assert ref.nll[0] == -np.log(1e-12) and ref.nll[1] == -np.log(1e-12)
    assert np.isfinite(ref.y).all() and (ref.y.astype(np.float32) == 0).any()
    # Wo = 0: one C-way exact tie everywhere
    ref = hr.head_ref(HL, hpre, np.zeros((4, 2), np.float32), [0, 1, 0], None, 1, SLOPE)
    assert ref.pred.tolist() == [0, 0, 0] and ref.undecided.size == 0
    assert hr.logit_rounding_bound(HL, Wo) == pytest.approx(2 * 3 * 2.0 ** -24 * (5 + 3 + 5) / 3)
