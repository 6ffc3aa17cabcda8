"""Forced kernel picks on the RECTANGULAR context.  The switch settings of tests/test_fuzz_shapes.py (the `runs`, `groups`, heavy-chunk,
bf16 group-sum and node-record forms of the source-major pass, chunked rows, tiny segments) have only ever met square contexts; here
each runs the lockstep harness of tests/shard_cases.py on parity_graph at P = 3 (n_table = 213 != n_rows = 10 / 69 / 71) with the NaN
poison on, for five shapes in both storage modes, against the one-GPU context under the same setting.  The switches are read once per
process: one subprocess per setting, five at a time (conftest.run_snippets_parallel)."""
import os
import textwrap

import pytest

from test_fuzz_shapes import SETTINGS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = """
    import sys
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import __graft_entry__ as entry
    import shard_cases as SC
    pkg = entry.load_package(); orc = entry.load_oracle()
    n = SC.pick_cases(pkg, orc, {tag!r})
    print("SWITCHES", pkg.abi.switches())
    print("OK cases", n)
"""
# gat_switches lists the switches the process READ and found set.  The phase API never reaches the fused last layer (gat_step only), so
# GAT_FUSE_LAST is not read here; the run length of the slot runs is read only where the runs form is the pick
STEP_ONLY = {"GAT_FUSE_LAST"}


@pytest.fixture(scope="module")
def pick_runs():
    from conftest import run_snippets_parallel
    jobs = {}
    for env, tag in SETTINGS:
        jobs[tag] = (textwrap.dedent(SNIPPET.format(root=ROOT, tests=os.path.join(ROOT, "tests"), tag=tag)), env)
    return run_snippets_parallel(jobs)


@pytest.mark.parametrize("env,tag", SETTINGS, ids=[t.strip() or "default" for _, t in SETTINGS])
def test_forced_picks_on_shards(pick_runs, env, tag):
    out = pick_runs[tag]
    assert out.returncode == 0 and "OK cases 10" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
    taken = dict(kv.split("=", 1) for kv in out.stdout.split("SWITCHES", 1)[1].splitlines()[0].split() if "=" in kv)
    for k, v in env.items():                   # the setting was really taken: read by the library, with this value
        if k not in STEP_ONLY:
            assert taken.get(k) == v, (k, v, taken)
    assert set(taken) <= set(env), taken       # and nothing else steered the run
