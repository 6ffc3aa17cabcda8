"""The lockstep shard harness (tests/shard_cases.py) on a machine without a GPU: the numpy stand-in of tests/fake_ctx.py in place of the HIP
contexts, the mixed-width model, the three graphs of the GPU cases at P = 2, 3, 4, against the literal oracle at 1e-4 (as
test_shard.py::test_fake_context_matches_oracle_single_rank).  What this shows without a GPU: the harness's exchange arithmetic, its row
maps (own rows, referenced rows, the stitched global order), the poison bookkeeping, and the conditions the GPU cases rely on."""
import numpy as np
import pytest

import parity
import shard_cases as SC


def _oracle(orc, g, heads, outdims):
    cfg = orc.Config(list(heads), list(outdims), g["f"], g["c"])
    P = orc.xavier_params(cfg, SC.PARAM_SEED)
    return cfg, P, orc.step(cfg, g["row_ptr"], g["col_idx"], g["labels"], g["x"], *P)


def _against_oracle(out, ref, cfg, g, tag):
    n = g["n"]
    assert abs(out["loss"] - ref.loss_sum_f64) < 1e-4 * n and out["correct"] == ref.n_correct, tag
    for name, got, want in zip(("gradW", "grada", "gradWo"), out["grads"], (ref.gradW, ref.grada, ref.gradWo)):
        parity.check_rel(f"{tag} {name}", got, want, 1e-4)
    st = SC.stitched(out, cfg.L, keep_taps=True)
    for l in range(cfg.L):                                   # the row maps: own rows of every rank, in the unsharded order
        parity.check_rel(f"{tag} hpre[{l}]", st["hpre"][l], ref.taps["hpre"][l], 1e-4)
        parity.check_rel(f"{tag} hout[{l}]", st["hout"][l], ref.taps["H"][l], 1e-4)
        parity.check_rel(f"{tag} alpha[{l}]", st["alpha"][l], ref.taps["alpha"][l], 1e-4)
        parity.check_rel(f"{tag} G[{l}]", st["G"][l], ref.taps["g"][l], 1e-4)
        parity.check_rel(f"{tag} galpha[{l}]", st["galpha"][l], ref.taps["galpha"][l], 1e-4)
        if l > 0:
            parity.check_rel(f"{tag} GX[{l}]", st["GX"][l], ref.taps["gx"][l], 1e-4)


@pytest.mark.parametrize("graph", list(SC.GRAPHS))
def test_plan_conditions(pkg, graph):
    """What the GPU cases rely on about the plans (tests/test_shard_shapes.py asserts the same before it trusts a case)."""
    make, world = SC.GRAPHS[graph]
    SC.check_plan(graph, SC.Shards(pkg.shard, make(), world))


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("graph", list(SC.GRAPHS))
def test_lockstep_harness_matches_oracle(pkg, orc, graph, world):
    """Mixed-width model, both input plans, full and halo all-gather, poison on: oracle at 1e-4; the poisoned step returns bit for bit
    what the unpoisoned one does; the halo form returns bit for bit what the full form does."""
    g = SC.GRAPHS[graph][0]()
    _, heads, outdims = SC.MIXED
    cfg, P, ref = _oracle(orc, g, heads, outdims)
    make_ctx, alloc = SC.fake_factory(heads, outdims, g)
    for replicate in (False, True):
        plain = SC.lockstep(pkg, g, world, heads, outdims, P, make_ctx, alloc, replicate=replicate, keep_taps=True)
        _against_oracle(plain, ref, cfg, g, f"{graph} P{world} rep{int(replicate)}")
        for halo in (False, True):
            out = SC.lockstep(pkg, g, world, heads, outdims, P, make_ctx, alloc, replicate=replicate, poison=True, halo=halo, keep_taps=True)
            SC.assert_same(out, plain, f"poisoned, halo={halo}")


def test_one_rank_is_the_square_case(pkg, orc):
    """world = 1: no exchange, n_table == n_rows — the form the GPU tests use as their one-GPU reference."""
    g = SC.GRAPHS["parity"][0]()
    _, heads, outdims = SC.MIXED
    cfg, P, ref = _oracle(orc, g, heads, outdims)
    make_ctx, alloc = SC.fake_factory(heads, outdims, g)
    out = SC.lockstep(pkg, g, 1, heads, outdims, P, make_ctx, alloc, keep_taps=True)
    _against_oracle(out, ref, cfg, g, "P1")


def test_poison_bookkeeping_catches_a_read_of_an_unreferenced_row(pkg, orc):
    """A stand-in whose edge forward touches every table row (a padded lane multiplied by zero) must fail the poisoned step."""
    from fake_ctx import FakeContext

    class Leaky(FakeContext):
        def layer_forward_edges(self, l):
            super().layer_forward_edges(l)
            tab = self.tables[(0, l)].reshape(self.n_table, self.hd[l]).astype(np.float64)
            self.hpre[l] = self.hpre[l] + 0.0 * tab.sum()

    g = SC.GRAPHS["parity"][0]()
    _, heads, outdims = SC.HD15
    cfg, P, ref = _oracle(orc, g, heads, outdims)
    import torch
    with pytest.raises(AssertionError, match="NaN in|is not finite"):
        SC.lockstep(pkg, g, 3, heads, outdims, P, lambda r: Leaky(heads, outdims, g["f"], g["c"]), lambda k: torch.zeros(k), poison=True)


def test_bf16_rounding_restatement():
    """to_bf16 is round-to-nearest-even: against torch's own conversion, ties and both signs included."""
    import torch
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 10.0 ** rng.integers(-6, 6, 4096).astype(np.float32),
                        np.array([1.00390625, 1.01171875, -1.00390625, 0.0, -0.0, 3.0e38], np.float32)])      # two exact ties
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(SC.to_bf16(a).view(np.uint32), want.view(np.uint32))
