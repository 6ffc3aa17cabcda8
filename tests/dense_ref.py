"""What the dense kernels (csrc/gat_gemm_kernels.hip) are held to, in numpy: the fp64 products of the same fp32 operands, the fp32
fma chain that is the yardstick (the reference's own per-edge loop is one), the bar, numpy models of the three-piece product, and
the guard bands around every buffer a launch may write.  Shared by tests/test_dense_precision.py (through a context),
tests/test_dense_seams.py (through the gat_op_dense_* seams) and tests/test_dense_cases_cpu.py (no GPU: the bar has teeth).

The bar.  With  ratio = max |got - exact| / sum_k |a_k| |b_k|  over all outputs and rc the same figure of the fp32 fma chain:
    ratio <= 1.5 * rc + 1e-7                       every case, every switch setting
    ratio <= 1e-6 * max(1, sqrt(K / 100))          default kernels with chains of at most 128 terms (or split-K), where rc meets it too
An output the kernel ADDS into, or multiplies by the LeakyReLU slope on its way out, gets one more fp32 rounding: 2^-24 |want|."""
import numpy as np

BOUND = 1e-6
ROUND = 2.0 ** -24
GUARD = 64                      # sentinel floats in front of and behind every buffer
SENTINEL = 0x7FC0DEAD           # a quiet NaN with a payload no kernel produces


def bf16_rne(x):
    """fp32 -> nearest bf16 (ties to even), as v_cvt_pk_bf16_f32 does for finite values; returned as fp32."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def _chain_ratio(a, b, exact, scale):
    """a [M,K], b [N,K] fp32: the error ratio of acc = fma(a_k, b_k, acc), k ascending, in fp32 (product exact, one rounding per step)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a64[:, k:k + 1] * b64[:, k][None, :]).astype(np.float32)
    return _ratio(acc, exact, scale)


def _ratio(got, exact, scale):
    return float(np.max(np.abs(got.astype(np.float64) - exact) / np.maximum(scale, 1e-300)))


def ratio_with_rounding(got, want, scale, roundings=0):
    """_ratio with `roundings` extra fp32 roundings of the result allowed (an accumulate, the slope multiply): 2^-24 |want| each."""
    if got.size == 0:
        return 0.0
    err = np.abs(got.astype(np.float64) - want) - roundings * ROUND * np.abs(want)
    return float(np.max(np.maximum(err, 0.0) / np.maximum(scale, 1e-300)))


def product(a, b):
    """a [M,K], b [N,K] fp32 -> (exact fp64 a b^T, scale = |a| |b|^T)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return a64 @ b64.T, np.abs(a64) @ np.abs(b64).T


def abs_bound(K):
    return BOUND * max(1.0, (K / 100) ** 0.5)


def chain_bound(rc):
    return 1.5 * rc + 1e-7


def draw(rng, shape, spread):
    """The input law of tests/test_dense_precision.py: normal values with magnitudes spread over 2^+-spread, so that low-order pieces
    of large values sit beside high-order pieces of small ones."""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-spread, spread + 1, shape))).astype(np.float32)


# ---- numpy models of the three-piece product (rowgemm_x3_kernel's mma: six bf16 MFMAs per 16 k, small terms first) -------------------
def split3(x):
    """split_pair's arithmetic: hi = bf16(x); mid = bf16(x - hi); lo = bf16((x - hi) - mid)."""
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_rne(r)
    return hi, mid, bf16_rne((r - mid).astype(np.float32))


PAIRS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))       # (piece of a, piece of b) in the kernels' order


def six_term(a, b, per_product=False):
    """The kernels' arithmetic on a [M,K], b [N,K]: per 16-k step six piece-pair MFMAs into one fp32 accumulator.  One rounding per MFMA
    (its 16 exact products summed exactly, then added), or — the pessimistic model — one rounding per product."""
    pa = [p.astype(np.float64) for p in split3(a)]
    pb = [p.astype(np.float64) for p in split3(b)]
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k0 in range(0, K, 16):
        for i, j in PAIRS:
            if per_product:
                for k in range(k0, min(k0 + 16, K)):
                    acc = (acc.astype(np.float64) + pa[i][:, k:k + 1] * pb[j][:, k][None, :]).astype(np.float32)
            else:
                acc = (acc.astype(np.float64) + pa[i][:, k0:k0 + 16] @ pb[j][:, k0:k0 + 16].T).astype(np.float32)
    return acc


def three_term(a, b):
    """hi*hi + hi*mid + mid*hi, summed exactly: the 2^-17-class "bf16x3" the kernels do NOT use."""
    pa = [p.astype(np.float64) for p in split3(a)]
    pb = [p.astype(np.float64) for p in split3(b)]
    return (pa[0] @ pb[0].T + pa[0] @ pb[1].T + pa[1] @ pb[0].T).astype(np.float32)


def bf16_once(a, b):
    """both operands rounded to bf16 once, the product summed exactly: one pass of the bf16 pipe."""
    return (bf16_rne(a).astype(np.float64) @ bf16_rne(b).astype(np.float64).T).astype(np.float32)


def dropped_last_step(a, b):
    """the exact product without its last 16-k step (a k loop that ends one step early)."""
    K = a.shape[1]
    last = ((K - 1) // 16) * 16
    return (a[:, :last].astype(np.float64) @ b[:, :last].astype(np.float64).T).astype(np.float32)


# ---- guard bands (GPU side: torch tensors) ---------------------------------------------------------------------------------------------
class Guarded:
    """A device buffer of `n` 4-byte words with GUARD sentinel words in front and behind.  `fill`: a numpy array of n words (float32 or
    int32 bit patterns), or None = sentinels in the body too (a launch must then write every cell it owns, and no other)."""

    def __init__(self, torch, n, fill=None):
        self.torch, self.n = torch, int(n)
        host = np.full(self.n + 2 * GUARD, SENTINEL, np.int32)
        if fill is not None:
            host[GUARD:GUARD + self.n] = np.ascontiguousarray(fill).reshape(-1).view(np.int32)
        self.before = host[GUARD:GUARD + self.n].copy()
        self.t = torch.from_numpy(host).to("cuda:0")

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def words(self):
        """(body as int32, guards intact?)"""
        host = self.t.cpu().numpy()
        ok = bool(np.all(host[:GUARD] == SENTINEL) and np.all(host[GUARD + self.n:] == SENTINEL))
        return host[GUARD:GUARD + self.n], ok

    def floats(self, shape=None):
        body, ok = self.words()
        assert ok, "a launch wrote into the guard band of one of its buffers"
        f = body.view(np.float32)
        return f if shape is None else f.reshape(shape)

    def untouched(self):
        body, ok = self.words()
        return ok and bool(np.array_equal(body, self.before))
