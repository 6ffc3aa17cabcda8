"""Every pair of step features on the GPU (include/gatv2_abi.h; the table, its constraints and the builder are tests/pair_cases.py, and
tests/test_feature_pairs_cpu.py proves on the host that every row is a fair case): each row of the pairwise covering table runs one
step on its own step path and is held to the fp64 model of tests/step_ref.py with the head of tests/head_model.py at the project's
bars — 1e-4 of max-abs, 1e-2 with bf16 storage — for the loss, the h_pre / hout / G taps, all ten gradient groups, the batch-norm
statistics and the head's own rows; a second context on gat_step must give the same bits; eval mode is held to the eval model.  The
whole table runs once per kernel-pick profile, in a child process of its own (the switches are read once per process).  Every pair
the library refuses is asserted to be refused, by the call, with the code and the text pair_cases.CONSTRAINTS states."""
import os
import textwrap

import pytest

import pair_cases as PC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIED = (124, 134, 137, 139)                              # a time limit, an abort, a kill, a segmentation fault (negative: a signal)

SNIPPET = """
    import signal, sys
    signal.alarm(400)
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import __graft_entry__ as entry
    import pair_cases as PC, parity
    pkg = entry.load_package()
    ok, failed = PC.run_table(pkg, {name!r})
    parity.flush()
    print("SWITCHES", pkg.abi.switches())
    print("OK rows", ok)
    sys.exit(1 if failed else 0)
"""


@pytest.fixture(scope="module")
def profile_runs():
    """{profile: CompletedProcess or None}: two children at a time.  After a child that died of a signal or ran into its time limit no
    further child is started: the profiles behind it have None."""
    from conftest import run_snippets_parallel
    names = list(PC.PROFILES)
    runs = dict.fromkeys(names)
    for k in range(0, len(names), 2):
        jobs = {name: (textwrap.dedent(SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name)), PC.PROFILES[name])
                for name in names[k:k + 2]}
        runs.update(run_snippets_parallel(jobs, workers=2, timeout=440))
        if any(r.returncode < 0 or r.returncode in DIED for r in runs.values() if r is not None):
            break
    return runs


@pytest.mark.parametrize("name", list(PC.PROFILES))
def test_table_under_the_profile(profile_runs, name):
    out, env = profile_runs[name], PC.PROFILES[name]
    assert out is not None, "not started: a child of an earlier profile died"
    failed = [ln for ln in out.stdout.splitlines() if ln.startswith("FAILED")]
    assert out.returncode == 0 and f"OK rows {len(PC.ROWS)}" in out.stdout, "\n".join(failed + [out.stdout[-1500:], out.stderr[-3000:]])
    taken = dict(kv.split("=", 1) for kv in out.stdout.split("SWITCHES", 1)[1].splitlines()[0].split() if "=" in kv)
    assert taken == env, (taken, env)


def _with(*levels):
    """PLAIN with the given (factor, level) pairs in place -> the builder's dict with seed-0 parameters."""
    lv = dict(zip(PC.NAMES, PC.PLAIN))
    lv.update(levels)
    st = dict(PC._static(tuple(lv[n] for n in PC.NAMES), "parity"))
    st["P"], st["inp"] = PC.params(st, 0)
    return st


@pytest.mark.parametrize("con", PC.CONSTRAINTS, ids=[f"{c[0][1]}-{c[1][1]}" for c in PC.CONSTRAINTS])
def test_constraint_is_a_refusal(pkg, con):
    """A context with exactly the pair is refused by the stated call with the stated code and text; with either level alone it is
    accepted and takes a step."""
    A = pkg.abi
    a, b, call, code, text = con
    calls = []

    class Traced(pkg.GatContext):
        def __getattribute__(self, name):
            if name.startswith("set_") or name.startswith("params_"):
                calls.append(name)
            return object.__getattribute__(self, name)
    with pytest.raises(A.GatError) as ei:
        PC.make_ctx(pkg, _with(a, b), cls=Traced)
    assert ei.value.code == code and text in str(ei.value) and calls[-1] == call, (str(ei.value), calls[-1])
    for alone in (a, b):
        with PC.make_ctx(pkg, _with(alone)) as ctx:
            loss, _ = ctx.step()
            assert loss == loss and loss != 0
