"""The batch-normalisation kernels through their two seams (gat_op_batch_norm_forward / _backward) against fp64 numpy
(bn_cases.kernel_model, pinned to torch.nn.BatchNorm1d by tests/test_batchnorm_cpu.py), at the smallest shapes at which they can go wrong:
n_rows in {1, 2, 63, 64, 65, 1500} x (H, D) in {(1,1), (1,7), (8,8), (2,4), (5,13), (20,13), (3,87)} — V = 1 and V = 4, a partly filled
last block, a row wider than 256 lanes at V = 1, rows of 1 to 64 lanes — each as a hidden and as the last layer, in training and in eval
mode.  Outputs and statistics at 1e-5 of max-abs (bn_cases.kernel_scales: and what the max-abs is of where a sum vanishes): fp32 sums of at most 1500 terms of spread ~1 carry a relative error of some
sqrt(1500) * 2^-24 = 2e-6 in the worst column (achieved: profiles/batch_norm/achieved_errors.json).  A column of mean 1e4 and unit spread
keeps var within 1e-3 relative, which a sum-of-squares implementation cannot.  The same table under GAT_RESIDENT_CAP = 1 and 3 in a
process of its own each (at 1500 rows every block walks several trips, with unequal counts under cap 3): twice, bitwise equal, and the
column vectors of the profiles within the same bound of each other."""
import os
import textwrap

import numpy as np
import pytest

import bn_cases as BC
import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("H,D", BC.SHAPES, ids=[f"h{h}_d{d}" for h, d in BC.SHAPES])
def test_seams_against_fp64(pkg, H, D):
    for case in BC.KERNEL_CASES:
        if case[1:3] == (H, D):
            a = BC.check_kernel_case(pkg, case)
            b = BC.run_kernel_case(pkg, case)
            assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a), BC.kernel_case_id(case)


def test_large_mean_column_keeps_its_variance(pkg):
    """Columns of mean 1e4 (and -1e4, and 0) and unit spread, 1500 rows: rstd — that is, var — within 1e-3 relative of fp64 on the fp32
    inputs; E[u^2] - mu^2 in fp32 has no digit left there (tests/test_batchnorm_cpu.py shows both)."""
    import torch
    A = pkg.abi
    n, H, D = 1500, 2, 4
    rng = np.random.default_rng(5)
    u = (rng.standard_normal((n, 8)) + np.array([1e4, -1e4, 0, 1e4, 1e4, 0, -1e4, 1e4])).astype(np.float32)
    u64 = u.astype(np.float64)
    var = ((u64 - u64.mean(0)) ** 2).mean(0)
    d_u = torch.from_numpy(u).cuda()
    ones, zeros = torch.ones(8, device="cuda"), torch.zeros(8, device="cuda")
    mr = torch.zeros((2, 8), device="cuda"); hout = torch.empty((n, 8), device="cuda")
    eps = 1e-5
    A.op_batch_norm_forward(d_u.data_ptr(), n, H, D, False, ones.data_ptr(), zeros.data_ptr(), eps, 0.01, 0.1, 0, 0, True, mr.data_ptr(), hout.data_ptr())
    got = mr.cpu().numpy().astype(np.float64)
    var_got = 1.0 / got[1] ** 2 - eps
    err = float((np.abs(var_got - var) / var).max())
    parity.record("var of a column of mean 1e4", err, 1e-3)
    assert err <= 1e-3, (var_got, var)
    parity.check_rel("mean of a column of mean 1e4", got[0], u64.mean(0), BC.KERNEL_TOL)      # the table's bar (an ulp of 1e4 is 1e-3)


def test_seam_errors(pkg):
    import torch
    A = pkg.abi
    t = torch.zeros((2, 64), device="cuda")
    p = t.data_ptr()
    fwd = lambda **k: A.op_batch_norm_forward(**dict(dict(d_u=p, n_rows=2, H=2, D=4, is_last=False, d_gamma=p, d_beta=p, eps=1e-5, slope=0.01, momentum=0.1,
                                                          d_running_mean=p, d_running_var=p, training=True, d_mean_rstd=p, d_hout=p), **k))
    bwd = lambda **k: A.op_batch_norm_backward(**dict(dict(d_u=p, d_g=p, d_gh=0, gh_stride=4, n_rows=2, H=2, D=4, d_gamma=p, d_beta=p, d_mean_rstd=p,
                                                           d_running_mean=p, d_running_var=p, eps=1e-5, slope=0.01, training=True, d_res=0, d_bias=0,
                                                           d_G=p, d_agg=0, d_grad_gamma=0, d_grad_beta=0, d_grad_b=0), **k))
    calls = [lambda: fwd(n_rows=0), lambda: fwd(H=0), lambda: fwd(d_u=0), lambda: fwd(d_hout=0), lambda: fwd(eps=0.0), lambda: fwd(momentum=1.5),
             lambda: fwd(eps=float("nan")), lambda: fwd(d_running_var=0), lambda: fwd(training=False, d_running_mean=0, d_running_var=0),
             lambda: fwd(d_mean_rstd=0), lambda: bwd(d_g=0), lambda: bwd(d_gh=p), lambda: bwd(d_g=0, d_gh=p, gh_stride=3), lambda: bwd(d_G=0),
             lambda: bwd(d_mean_rstd=0), lambda: bwd(training=False, d_running_var=0), lambda: bwd(n_rows=-1)]
    for i, call in enumerate(calls):
        with pytest.raises(A.GatError) as ei:
            call()
        assert ei.value.code == 10001, i
    fwd(d_running_mean=0, d_running_var=0)               # training without running statistics: allowed, nothing is updated
    bwd()


SNIPPET = """
    import signal, sys
    signal.alarm(240)
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import __graft_entry__ as entry
    import bn_cases as BC, parity
    parity.set_test("tests/test_batchnorm_kernels.py::test_table_under_the_profile[{name}]")
    pkg = entry.load_package()
    n, failures = BC.run_kernel_profile(pkg, {outdir!r})
    parity.flush()
    print("SWITCHES", pkg.abi.switches())
    print("OK cases", n - len(failures))
    sys.exit(1 if failures else 0)
"""


@pytest.fixture(scope="module")
def profile_runs(tmp_path_factory):
    from conftest import run_snippets_parallel
    dirs = {name: str(tmp_path_factory.mktemp(name)) for name in BC.PROFILES}
    jobs = {name: (textwrap.dedent(SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name, outdir=dirs[name])), env)
            for name, env in BC.PROFILES.items()}
    return run_snippets_parallel(jobs, workers=2, timeout=270), dirs


@pytest.mark.parametrize("name", list(BC.PROFILES))
def test_table_under_the_profile(profile_runs, name):
    out, env = profile_runs[0][name], BC.PROFILES[name]
    failed = [ln for ln in out.stdout.splitlines() if ln.startswith("FAILED")]
    assert out.returncode == 0 and f"OK cases {len(BC.KERNEL_CASES)}" in out.stdout, "\n".join(failed + [out.stdout[-1500:], out.stderr[-3000:]])
    taken = dict(kv.split("=", 1) for kv in out.stdout.split("SWITCHES", 1)[1].splitlines()[0].split() if "=" in kv)
    assert taken == env, (taken, env)


def test_profiles_agree_within_the_bound(profile_runs):
    """The column vectors (statistics, the three parameter gradients) of cap 1 against cap 3: other grids, other summation orders, the
    same bound."""
    runs, dirs = profile_runs
    assert all(r.returncode == 0 for r in runs.values())
    a, b = (np.load(os.path.join(dirs[name], "vectors.npz")) for name in ("cap1", "cap3"))
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 0
    differ = 0
    for k in a.files:
        if k.endswith(" scale"):
            continue
        assert np.abs(a[k].astype(np.float64) - b[k]).max() <= BC.KERNEL_TOL * float(a[k + " scale"]), k      # (bn_cases.kernel_scales)
        differ += not np.array_equal(a[k], b[k])
    assert differ > 0                                    # the profiles did run different grids
