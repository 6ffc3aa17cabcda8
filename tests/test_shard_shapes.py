"""The kernels at the SHARD shape: every fast-path shape in both storage modes and the generic models on rectangular contexts
(n_table != n_rows, table_row0 != 0, referenced rows sparse, padding rows nobody wrote, ranks without an edge), driven by the lockstep
harness of tests/shard_cases.py and held to the ONE-GPU result of the same model, storage mode and keep_taps — which is itself held to
the oracle in the same test.  Forward: bitwise (the loss excepted, see shard_cases.check_forward); backward: 1e-5 of max-abs (bf16 below
the last layer: 1e-2); reproducibility: bitwise for the fast-path models; and a poisoned step — NaN in every table row no edge
references — must return bit for bit what the clean step returns."""
import pytest

import feature_cases as FC
import shard_cases as SC

pytestmark = pytest.mark.gpu

MODELS = [(SC.shape_name(hd, d), *SC.shape_heads(hd, d), dt, (hd, d) in SC.SMALL_SHAPES) for hd, d in FC.SHAPES for dt in FC.DTYPES] + \
         [(name, heads, outdims, "fp32", name == "hd15") for name, heads, outdims in SC.GENERIC]
POISON = [(SC.shape_name(hd, d), *SC.shape_heads(hd, d), dt) for hd, d in [(64, 8), (32, 8), (16, 4), (8, 8)] for dt in FC.DTYPES] + \
         [(*SC.HD15, "fp32")]


def _fast(heads, outdims):
    return all((h * d, d) in FC.SHAPES for h, d in zip(heads, outdims))


def _run(pkg, orc, graph, name, heads, outdims, dtype, keep_taps, **kw):
    g, cfg, P, _ = SC.oracle_case(orc, graph, name, heads, outdims)
    make_ctx, alloc, stream = SC.hip_factory(pkg, heads, outdims, g, dtype, keep_taps)
    return SC.lockstep(pkg, g, SC.GRAPHS[graph][1], heads, outdims, P, make_ctx, alloc, keep_taps=keep_taps, stream=stream, **kw)


@pytest.mark.parametrize("name,heads,outdims,dtype,small", MODELS, ids=[f"{m[0]}-{m[3]}" for m in MODELS])
def test_shard_equals_one_gpu(pkg, orc, name, heads, outdims, dtype, small):
    fast = _fast(heads, outdims)
    for graph in SC.GRAPHS if small else ["parity"]:
        g, cfg, P, _ = SC.oracle_case(orc, graph, name, heads, outdims)
        SC.check_plan(graph, SC.Shards(pkg.shard, g, SC.GRAPHS[graph][1]))
        for keep_taps in (False, True):
            one = SC.one_gpu(pkg, orc, graph, name, heads, outdims, dtype, keep_taps)
            for replicate in (False, True):
                tag = f"{graph} rep={int(replicate)} taps={int(keep_taps)}:"
                out = _run(pkg, orc, graph, name, heads, outdims, dtype, keep_taps, replicate=replicate)
                st, ost = SC.check_forward(tag, out, one, cfg.L, keep_taps)
                SC.check_backward(tag, out, one, cfg, dtype, keep_taps, st, ost)
                again = _run(pkg, orc, graph, name, heads, outdims, dtype, keep_taps, replicate=replicate)
                if fast:                                     # reproducibility: fixed-order sums everywhere
                    SC.assert_same(again, out, tag + " second run")
                else:
                    SC.assert_same_forward_close_backward(again, out, tag + " second run")


@pytest.mark.parametrize("name,heads,outdims,dtype", POISON, ids=[f"{m[0]}-{m[3]}" for m in POISON])
def test_poisoned_step_equals_clean_step(pkg, orc, name, heads, outdims, dtype):
    """No kernel may read a table row no edge of the shard references: the halo form and a bound table promise nothing about those rows.
    NaN bit patterns in all of them (PL), and in the whole gPL table before every edge backward: the same results bit for bit, every gPL
    row of an unreferenced source exactly 0.0, every referenced one finite (asserted inside the harness)."""
    fast = _fast(heads, outdims)
    for graph in SC.GRAPHS:
        for replicate, halo in ((False, False), (False, True), (True, True)):
            clean = _run(pkg, orc, graph, name, heads, outdims, dtype, False, replicate=replicate, halo=halo)
            dirty = _run(pkg, orc, graph, name, heads, outdims, dtype, False, replicate=replicate, halo=halo, poison=True)
            what = f"{graph} rep={int(replicate)} halo={int(halo)}: poisoned vs clean"
            (SC.assert_same if fast else SC.assert_same_forward_close_backward)(dirty, clean, what)
