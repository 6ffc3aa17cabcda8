"""The persistent kernels when a block walks many items: every grid that is sized by the resident count — the edge backward family, the
fused last layer, res_backward / norm_backward, the softmax and BCE / MSE heads, the two kernels of the hidden head layer — under
GAT_RESIDENT_CAP = 1 and 3, where a graph of a few hundred rows makes each wave walk several trips (cap 3: unequal trip counts), held to
the fp64 models and the bars of the feature tests they come from: 1e-4 of max-abs for fp32, 1e-2 for bf16 storage against the model
with bf16_pl, the alpha tap and the DropEdge mask bit for bit with keep_taps, the head tests' own bounds, the hidden layer's seams
bitwise.  Uncapped, these loops run at most once on every graph of the suite, and the full-size tests walk them with the plain model
only.  tests/trip_cases.py has the profiles, graphs and tables; tests/test_grid_trips_cpu.py proves that the trips happen and that
every case has a seed.

The switches are read once per process: one subprocess per profile (conftest.run_snippets_parallel); each computes its own fp64 models."""
import os
import textwrap

import pytest

import trip_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = """
    import signal, sys
    signal.alarm({limit})                        # the profile's own time limit: the default action ends the process
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import __graft_entry__ as entry
    import trip_cases as TC
    pkg = entry.load_package(); orc = entry.load_oracle()
    n, failures = TC.run_profile(pkg, orc, {name!r})
    print("SWITCHES", pkg.abi.switches())
    print("OK cases", n - len(failures))
    sys.exit(1 if failures else 0)
"""


@pytest.fixture(scope="module")
def profile_runs():
    from conftest import run_snippets_parallel
    jobs = {name: (textwrap.dedent(SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name, limit=TC.TIMEOUT[name])), env)
            for name, env in TC.PROFILES.items()}
    return run_snippets_parallel(jobs, workers=4, timeout=max(TC.TIMEOUT.values()) + 30)


@pytest.mark.parametrize("name", list(TC.PROFILES))
def test_every_case_under_the_profile(profile_runs, name):
    out, env = profile_runs[name], TC.PROFILES[name]
    failed = [ln for ln in out.stdout.splitlines() if ln.startswith("FAILED")]       # each names profile and case
    want = len(TC.table(name))
    assert out.returncode == 0 and f"OK cases {want}" in out.stdout, "\n".join(failed + [out.stdout[-1500:], out.stderr[-3000:]])
    taken = dict(kv.split("=", 1) for kv in out.stdout.split("SWITCHES", 1)[1].splitlines()[0].split() if "=" in kv)
    assert taken == env, (taken, env)            # the cap (and the profile's other switches) was read, and nothing else steered the run
