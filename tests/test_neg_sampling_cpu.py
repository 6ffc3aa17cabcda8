"""synth.negative_pairs — the numpy statement of the sampling law of include/gatv2_abi.h "negative sampling" — against a brute-force
Python set of the edges, on the host.  Also the condition tests/test_neg_sampling.py relies on: on the ascending fixture in UNIFORM mode
no negative of any (count, round) it runs is unfiltered, so a GPU comparison there exercises the filter and not the fall-back."""
import numpy as np
import pytest

import neg_cases as NC


@pytest.fixture(scope="module")
def graphs(pkg):
    out = {}
    for variant in NC.VARIANTS:
        rp, ci = NC.fixture_graph(pkg, variant)
        out[variant] = (rp, ci, NC.edge_set(rp, ci))
    return out


def test_fixture_graphs(pkg, graphs):
    rp, ci, edges = graphs["ascending"]
    deg = np.diff(rp)
    assert deg[:10].tolist() == NC.DEGREES
    assert sorted(ci[rp[NC.HUB]:rp[NC.HUB + 1]].tolist()) == [i for i in range(NC.N) if i != NC.HUB]
    assert 3 <= deg[10:].min() and deg[10:].max() <= 7 and abs(deg[10:].mean() - 5.0) < 0.5
    assert 0.02 < len(ci) / NC.N ** 2 < 0.04
    asc = lambda rp, ci: all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) >= 0) for r in range(NC.N))
    assert asc(rp, ci) and len(edges) == len(ci)
    rs, cs, es = graphs["shuffled"]
    assert not asc(rs, cs) and es == edges and np.array_equal(rs, rp)
    rd, cd, ed = graphs["duplicates"]
    assert asc(rd, cd) and ed == edges and len(cd) > len(ci)


@pytest.mark.parametrize("flags", NC.FLAGS)
@pytest.mark.parametrize("mode", (NC.UNIFORM, NC.CORRUPT))
@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_law_against_the_edge_set(pkg, graphs, variant, mode, flags):
    S = pkg.synth
    rp, ci, edges = graphs[variant]
    su, sv = NC.sources(pkg, rp, ci)
    kw = dict(src_u=su, src_v=sv) if mode == NC.CORRUPT else {}
    count = 1000
    prev = None
    for rnd in NC.ROUNDS:
        u, v, unf = S.negative_pairs(rp, ci, mode, count, NC.SEED, rnd, flags, **kw)
        assert u.dtype == np.int32 and v.dtype == np.int32 and u.shape == v.shape == (count,)
        assert u.min() >= 0 and v.min() >= 0 and u.max() < NC.N and v.max() < NC.N
        bad = NC.fails(edges, u, v, flags)
        assert unf == int(bad.sum())                     # accepted negatives pass the rule; the others are the unfiltered ones
        if not flags & NC.SELF:
            assert np.all((u != v) | bad)
        if mode == NC.CORRUPT:
            role = NC.roles(pkg, NC.SEED, rnd, count)
            p = np.arange(count) % len(su)
            assert np.array_equal(v[role == 0], sv[p][role == 0]) and np.array_equal(u[role == 1], su[p][role == 1])
            assert 0.4 < role.mean() < 0.6
        u2, v2, unf2 = S.negative_pairs(rp, ci, mode, count, NC.SEED, rnd, flags, **kw)
        assert np.array_equal(u, u2) and np.array_equal(v, v2) and unf == unf2
        if prev is not None:
            assert ((u != prev[0]) | (v != prev[1])).mean() > 0.5
        prev = (u, v)
    us, vs, _ = S.negative_pairs(rp, ci, mode, count, NC.SEED + 1, 0, flags, **kw)        # another seed: another list
    u0, v0, _ = S.negative_pairs(rp, ci, mode, count, NC.SEED, 0, flags, **kw)
    assert ((us != u0) | (vs != v0)).mean() > 0.5


def test_the_result_does_not_depend_on_the_row_order(pkg, graphs):
    """The three variants hold the same edge set: the same negatives."""
    S = pkg.synth
    base = None
    for variant in NC.VARIANTS:
        rp, ci, _ = graphs[variant]
        got = S.negative_pairs(rp, ci, NC.UNIFORM, 1000, NC.SEED, 3, NC.BOTH)
        if base is not None:
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[2] == base[2]
        base = got


def test_condition_no_unfiltered_negative_on_the_sparse_fixture(pkg, graphs):
    """Edge density about 0.03, 16 tries: exhaustion has probability about 1e-24 per negative.  Asserted, not assumed."""
    rp, ci, _ = graphs["ascending"]
    for flags in NC.FLAGS:
        for count in NC.COUNTS + (1200,):
            for rnd in NC.ROUNDS:
                assert pkg.synth.negative_pairs(rp, ci, NC.UNIFORM, count, NC.SEED, rnd, flags)[2] == 0, (flags, count, rnd)


def test_exhaustion_is_counted(pkg, graphs):
    """Sources that all end at the hub: a role-0 negative (w, hub) is an edge or the self pair on every attempt."""
    S = pkg.synth
    rp, ci, edges = graphs["ascending"]
    su, sv = NC.hub_sources()
    for flags in NC.FLAGS:
        u, v, unf = S.negative_pairs(rp, ci, NC.CORRUPT, 1000, NC.SEED, 1, flags, src_u=su, src_v=sv)
        role = NC.roles(pkg, NC.SEED, 1, 1000)
        bad = NC.fails(edges, u, v, flags)
        assert unf == int(bad.sum()) and not np.any(bad[role == 1])
        if flags & NC.SELF:                              # (hub, hub) is no edge: accepted once w hits the hub — rarely within 16 tries
            assert np.all(bad[role == 0] | (u[role == 0] == NC.HUB))
            assert unf > 0.8 * int((role == 0).sum())
        else:
            assert unf == int((role == 0).sum())


def test_degenerate_graphs(pkg):
    S = pkg.synth
    rp, ci = NC.complete_graph(4)
    for mode, kw in ((NC.UNIFORM, {}), (NC.CORRUPT, dict(src_u=np.array([0, 1], np.int32), src_v=np.array([2, 3], np.int32)))):
        for flags in NC.FLAGS:
            u, v, unf = S.negative_pairs(rp, ci, mode, 65, NC.SEED, 2, flags, **kw)
            assert unf == 65 and u.max() < 4 and v.max() < 4
    rp, ci = NC.single_node()
    for flags in NC.FLAGS:
        u, v, unf = S.negative_pairs(rp, ci, NC.UNIFORM, 65, NC.SEED, 0, flags)
        assert np.all(u == 0) and np.all(v == 0)
        assert unf == (0 if flags & NC.SELF else 65)


def test_bad_arguments(pkg):
    S = pkg.synth
    rp, ci = NC.complete_graph(4)
    for args in ((0, 5), (3, 5), (NC.UNIFORM, 0)):
        with pytest.raises(ValueError):
            S.negative_pairs(rp, ci, args[0], args[1], 1, 0)
    with pytest.raises(ValueError):
        S.negative_pairs(rp, ci, NC.UNIFORM, 5, 1, 0, flags=4)
    with pytest.raises(ValueError):
        S.negative_pairs(rp, ci, NC.CORRUPT, 5, 1, 0)
