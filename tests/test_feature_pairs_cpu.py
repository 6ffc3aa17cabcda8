"""The table of tests/pair_cases.py on the host, before any kernel is involved: it covers every pair of levels that is not a constraint
and holds no constrained pair, the generator reproduces it, every committed seed is clear of the kinks on the fp64 model (and is the
first such seed), no row's reference vanishes, and the fallback graph stays the exception."""
import numpy as np
import pytest

import pair_cases as PC
import step_ref as SR

N = len(PC.NAMES)
IDS = [PC.row_id(i) for i in range(len(PC.ROWS))]


def test_the_table_covers_every_pair():
    covered = set()
    for row in PC.ROWS:
        pairs = PC.row_pairs(row[:N])
        assert not any(PC.refused(a, b) for a, b in pairs), row
        covered.update(pairs)
    want = set(PC.all_pairs())
    assert want <= covered, sorted(want - covered)[:5]
    # every pair of levels of two different factors is in `want` or in CONSTRAINTS, and the two do not overlap
    total = sum(len(li) * len(lj) for i, (_, li) in enumerate(PC.FACTORS) for _, lj in PC.FACTORS[i + 1:])
    assert len(want) + len(PC.CONSTRAINTS) == total and len({frozenset(c[:2]) for c in PC.CONSTRAINTS}) == len(PC.CONSTRAINTS)
    levels = {(f, lv) for f, lvs in PC.FACTORS for lv in lvs}
    assert all(c[0] in levels and c[1] in levels and c[0][0] != c[1][0] for c in PC.CONSTRAINTS)


def test_the_generator_gives_the_committed_table():
    assert tuple(PC.generate()) == tuple(row[:N] for row in PC.ROWS)
    assert 36 <= len(PC.ROWS) <= 70 and f"({len(PC.ROWS)} rows" in PC.__doc__


def test_one_row_is_what_the_fused_last_layer_takes():
    """GAT_FUSE_LAST=1 must fuse the plain records_d8 / fp32 / softmax / node row, on gat_step, and no other row."""
    fused = [i for i, row in enumerate(PC.ROWS) if PC.fused_eligible(PC.levels_of(row))]
    assert fused == [0] and PC.ROWS[0][:N] == PC.PLAIN and PC.levels_of(PC.ROWS[0])["path"] == "step"


def test_the_fallback_graph_stays_the_exception():
    """At least four rows in five run on parity_graph; "small" is taken only where no seed below 400 is clear on the row's first graph
    (test_seed_is_the_first_clear_one re-checks that for the rows it visits)."""
    on_parity = [row for row in PC.ROWS if row[-1] == "parity" and PC._static(tuple(row[:N]), "parity")["g"]["n"] == 150]
    assert all(row[-1] in ("parity", "small") for row in PC.ROWS)
    assert 5 * len(on_parity) >= 4 * len(PC.ROWS), (len(on_parity), len(PC.ROWS))


@pytest.mark.parametrize("i", range(len(PC.ROWS)), ids=IDS)
def test_seed_is_clear(i):
    st = PC.case(i)
    assert 0 <= st["seed"] < PC.BC.SEEDS and PC.clear(st, st["ref"])


@pytest.mark.parametrize("i", range(0, len(PC.ROWS), 5), ids=IDS[::5])
def test_seed_is_the_first_clear_one(i):
    row = PC.ROWS[i]
    assert not any(PC.seed_is_clear(row[:N], row[-1], s) for s in range(row[-2]))
    if row[-1] == "small":
        assert PC.first_clear_seed(row[:N], "parity") is None


def test_fallback_rows_have_no_clear_seed_on_their_first_graph():
    for row in PC.ROWS:
        if row[-1] == "small":
            assert PC.first_clear_seed(row[:N], "parity") is None, row


@pytest.mark.parametrize("i", range(len(PC.ROWS)), ids=IDS)
def test_reference_does_not_vanish(i):
    """Loss, every gradient group the row has and every layer's G are non-zero; a group it does not have is None.  (gamma / beta of a
    one-layer skip_last row are never read: their gradient is exactly 0, which the GPU test asserts.)"""
    st = PC.case(i)
    ref, lv = st["ref"], st["lv"]
    assert ref["loss"].item() != 0
    has = dict(W=True, a=True, Wo=True, Wres=st["lin"], b=st["bias"], gamma=st["normed"], beta=st["normed"], We=st["fe"] > 0,
               W1=st["dh"] > 0, b1=st["dh"] > 0)
    dead = st["normed"] and st["skip_last"] and st["cfg"].L == 1
    for k in SR.GROUPS:
        if not has[k]:
            assert ref[k] is None, k
        elif dead and k in ("gamma", "beta"):
            assert ref[k].grad is None or not ref[k].grad.numpy().any()
        elif k == "b" and st["bn"] and not st["skip_last"]:
            assert ref[k].grad is not None               # sum_n G[n,c]: identically 0 behind a batch norm (bn_cases.compare)
        else:
            assert np.abs(ref[k].grad.numpy()).max() > 0, (k, lv)
    for l in range(st["cfg"].L):
        assert ref["hpre"][l].grad.abs().max().item() > 0, l
    assert np.isfinite(st["eval_ref"]["loss"].item())
