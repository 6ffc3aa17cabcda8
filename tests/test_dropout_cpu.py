"""Dropout without a GPU: the mask hash of include/gatv2_abi.h ("dropout") restated in numpy, the new ABI symbols, and the
train_edge flags' argument errors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dropout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "graph-attention-network-gatv2-_amd", "train_edge")
NEW_SYMBOLS = ["gat_set_dropout", "gat_set_training", "gat_dropout_step", "gat_set_shard_bounds"]


def test_fmix32_known_values():
    # MurmurHash3's 32-bit finaliser: 0 is a fixed point; spot values computed with plain Python integers
    def ref(h):
        h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF; h ^= h >> 16
        return h
    xs = np.array([0, 1, 2, 0xDEADBEEF, 0xFFFFFFFF, 12345678], np.uint64)
    assert [int(v) for v in R.fmix32(xs)] == [ref(int(x)) for x in xs]
    assert int(R.fmix32(0)) == 0
    assert int(R.mix(7, 9)) == ref(7 ^ ((9 * 0x9E3779B9 + 0x7F4A7C15) & 0xFFFFFFFF))


def test_threshold_and_scale():
    assert R.threshold(0.0) == 0 and R.threshold(0.5) == 1 << 23
    assert R.threshold(0.999999999) == 1 << 24
    assert R.scale(0.5) == np.float32(2.0) and R.scale(0.0) == np.float32(1.0)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate_within_5_sigma(p):
    n = 1_000_000
    r = R.mix(R.key(11, 3, 0, 1), np.arange(n))
    rate = R.keep(r, p).mean()
    want = 1.0 - R.threshold(p) / 2.0 ** 24
    sigma = np.sqrt(want * (1 - want) / n)
    assert abs(rate - want) < 5 * sigma, (rate, want, sigma)


def test_masks_differ_across_seed_step_layer_kind_head():
    rp = np.array([0, 40, 90, 200], np.int64)
    base = R.attn_factor(1, 0, 0, rp, 2, 0.5)
    assert not np.array_equal(base, R.attn_factor(2, 0, 0, rp, 2, 0.5))       # seed
    assert not np.array_equal(base, R.attn_factor(1, 1, 0, rp, 2, 0.5))       # step
    assert not np.array_equal(base, R.attn_factor(1, 0, 1, rp, 2, 0.5))       # layer
    assert not np.array_equal(base[0], base[1])                              # head
    assert R.key(1, 0, 0, 0) != R.key(1, 0, 0, 1)                             # kind
    f = R.feat_factor(1, 0, 0, 3, 200, 0.5)
    assert not np.array_equal(f.ravel(), base[0])
    # high words of seed and step take part
    assert R.key(1, 0, 0, 1) != R.key(1 + (1 << 32), 0, 0, 1) and R.key(1, 0, 0, 1) != R.key(1, 1 << 32, 0, 1)
    # factors are exactly 0 or 1/(1-p)
    assert set(np.unique(base)) <= {np.float32(0), np.float32(2)}


def test_shard_node_ids_give_the_single_gpu_masks():
    """A shard keys its rows by their unsharded ids: the masks of rows [lo, hi) drawn with nodes = lo.. equal the rows of the
    whole graph's masks."""
    rng = np.random.default_rng(0)
    deg = rng.integers(0, 30, 50)
    rp = np.concatenate([[0], np.cumsum(deg)])
    whole = R.attn_factor(5, 2, 1, rp, 4, 0.3)
    lo, hi = 17, 41
    part = R.attn_factor(5, 2, 1, rp[lo:hi + 1] - rp[lo], 4, 0.3, nodes=np.arange(lo, hi))
    assert np.array_equal(part, whole[:, rp[lo]:rp[hi]])


def test_new_symbols_declared_and_exported(pkg):
    A = pkg.abi
    names = A.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in names
    lib = ctypes.CDLL(A.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert A.TAP_ATTN_KEEP == 15 and A.TAP_FEAT_KEEP == 16
    assert A.load_library().gat_abi_version() == 6


@pytest.mark.parametrize("flag,value", [("--attn-dropout", "1.0"), ("--dropout", "-0.1"), ("--dropout", "nan"), ("--attn-dropout", "x")])
def test_train_edge_refuses_bad_dropout(flag, value):
    e = dict(os.environ)
    e.pop("DATA_ROOT", None)
    r = subprocess.run([BIN, "--heads", "8,8", "--outdims", "8,8", flag, value], capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 1
    assert r.stderr.endswith(f"Error: {flag} must be in [0, 1)\n"), r.stderr
    assert "[Memory Tracker]" not in r.stdout                # refused before anything touches the GPU
