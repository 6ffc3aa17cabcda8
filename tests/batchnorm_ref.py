"""What batch normalisation (include/gatv2_abi.h "batch normalisation") needs beside the step model of tests/step_ref.py (bn=True): the
statistics of a fresh context, the running-statistics law, and a numpy restatement of the kernels' Welford / Chan merge."""
import numpy as np

from step_ref import ln_offsets


def stats_init(cfg):
    """(running_mean, running_var) of a fresh context: 0 and 1, flat [l][H_l*D_l]."""
    n = ln_offsets(cfg)[-1]
    return np.zeros(n), np.ones(n)


def running_update(run_mean, run_var, mu, var, n, momentum):
    """The running-statistics law on numpy arrays (var: the biased batch variance)."""
    unbiased = var * n / (n - 1) if n > 1 else var
    return (1 - momentum) * run_mean + momentum * mu, (1 - momentum) * run_var + momentum * unbiased


def welford_chan(u, chunks):
    """numpy restatement of the kernels' merge in fp64: per chunk of rows a Welford pass, the chunks folded in ascending order with Chan's
    formula.  u [N][C], chunks: list of row-index arrays (a partition of the rows).  -> (mean [C], biased var [C])."""
    n, m, q = 0.0, None, None
    for rows in chunks:
        if len(rows) == 0:
            continue
        nb, mb, qb = 0.0, np.zeros(u.shape[1]), np.zeros(u.shape[1])
        for r in rows:
            nb += 1.0
            d = u[r] - mb
            mb = mb + d / nb
            qb = qb + d * (u[r] - mb)
        if n == 0.0:
            n, m, q = nb, mb, qb
            continue
        tot = n + nb
        delta = mb - m
        m = m + delta * (nb / tot)
        q = q + qb + delta * delta * (n * (nb / tot))
        n = tot
    return m, q / n
