"""The feature forms of the edge kernels — dropout, DropEdge, residual / bias, layer norm, edge features, their bf16-storage and keep_taps
forms — against fp64 under the kernel picks of the FULL-SIZE shapes.  The graphs of the suite have a few thousand edges, so their rows
are cut into segments of 16 (build_worklist): the group-per-row kernels walk items of at most four steps and close only such rows in
their epilogue, and the source-major pass is the list pull without node records.  The full-size shapes run segments of 32 / 64 / 256,
the slot-parallel pull and the last layer's node records.  Each profile of tests/pick_profiles.py sets the switches that give a small
graph the defaults of one BASELINE shape and runs the whole case table (48 steps) on long_rows_graph — rows of 15 .. 257 in-edges, a
hub source of more than 256 slots — at the project's bars: 1e-4 of max-abs for fp32, 1e-2 for bf16 storage against the model with
bf16_pl; with keep_taps also the alpha tap, the DropEdge mask bit for bit and exact zeros at the dropped edges.
tests/test_full_size_picks_cpu.py derives the profiles from the rules and proves what the graph, the masks and the seeds must offer.

The switches are read once per process: one subprocess per profile (conftest.run_snippets_parallel); each computes the fp64 models
itself (about two seconds for all 46 on this graph)."""
import os
import textwrap

import pytest

import pick_profiles as PP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = """
    import sys
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import __graft_entry__ as entry
    import pick_profiles as PP
    pkg = entry.load_package(); orc = entry.load_oracle()
    n, failures = PP.run_profile(pkg, orc, {name!r})
    print("SWITCHES", pkg.abi.switches())
    print("OK cases", n - len(failures))
    sys.exit(1 if failures else 0)
"""


@pytest.fixture(scope="module")
def profile_runs():
    from conftest import run_snippets_parallel
    jobs = {name: (textwrap.dedent(SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name)), env)
            for name, env in PP.PROFILES.items()}
    return run_snippets_parallel(jobs, workers=4)


@pytest.mark.parametrize("name", list(PP.PROFILES))
def test_feature_forms_under_the_profile(profile_runs, name):
    out, env = profile_runs[name], PP.PROFILES[name]
    failed = [ln for ln in out.stdout.splitlines() if ln.startswith("FAILED")]       # each names profile, model, storage mode and form
    assert out.returncode == 0 and f"OK cases {len(PP.CASES)}" in out.stdout, "\n".join(failed + [out.stdout[-1500:], out.stderr[-3000:]])
    taken = dict(kv.split("=", 1) for kv in out.stdout.split("SWITCHES", 1)[1].splitlines()[0].split() if "=" in kv)
    assert taken == env, (taken, env)            # every switch of the profile was read with its value, and nothing else steered the run
