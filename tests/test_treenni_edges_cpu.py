"""The edges of phylo_trees_nni without a GPU (inputs: trees_edges_cases.py): the restatement against the
same formulas at 50 digits on trees of 129 to 512 taxa (E_NNI_BIG, E_EXPL_BIG: the error grows with a caterpillar's depth, and
the bounds of the small trees do not cover it), the move sample of the explicit comparison, apply_nni at 129 and 512 taxa, and
every precondition that test_gpu_treenni_edges.py asserts again before it compares anything: site factors clear of the floor, the
NaN and -inf patterns of the big cases, the scaled sites, the random columns over 300 and 310 taxa."""
import functools

import numpy as np
import pytest

import treegrad_ref as TR
import treenni_cases as NC
import treenni_ref as NR
import trees_edges_cases as EC
from phylo_amd.treesearch import apply_nni, nni_moves
from test_gpu_treenni import missing_moves
from test_gpu_trees_loglik import bits
from treegrad_cases import branch_matrices
from treenni_cases import E_EXPL_BIG, E_NNI_BIG, PRIOR, TOL_EXPL_BIG
from trees_edges_cases import FLOOR, ROOMY

S_MP = 6                                 # sites of the 50-digit comparison, cut from the front of the case's alignment


# ---- the restatement at 50 digits on deep trees: E_NNI_BIG, E_EXPL_BIG ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measured(name):
    mp = pytest.importorskip("mpmath")
    g, child, blen, Q = EC.big_case(name)
    return NC.measure_deep(mp, child, blen, Q, PRIOR, g[:, :S_MP])


@pytest.mark.parametrize("name", list(EC.BIG))
def test_reference_against_mpmath_big(name):
    """All five trees of the case, the first 6 sites.  E_NNI_BIG over EVERY move, E_EXPL_BIG over treenni_cases.move_sample, in
    the units of test_treenni_cpu.py::test_reference_against_mpmath.  An impossible neighbour is -inf in the restatement where
    the 50-digit L' is exactly zero (asserted inside measure_deep, for the explicit tree too).  Measured: see treenni_cases.py."""
    worst_n, worst_x, seen, dead = measured(name)
    print("%s: restatement against 50 digits over %d moves (%d impossible): delta %.3f units (E_NNI_BIG = %g), explicit neighbours "
          "%.3f units (E_EXPL_BIG = %g)" % (name, seen, dead, worst_n, E_NNI_BIG, worst_x, E_EXPL_BIG))
    N = EC.BIG[name]['N']
    assert seen >= 5 * 2 * (N - 2)
    if EC.BIG[name]['shape'] == 'caterpillar':
        assert dead >= 1
    assert worst_n <= E_NNI_BIG
    assert worst_x <= E_EXPL_BIG


def test_big_bounds_are_not_stale():
    """over the whole set the worst errors lie above half the bounds: a constant left behind by a change of the cases fails"""
    res = [measured(name) for name in EC.BIG]
    worst_n, worst_x = max(r[0] for r in res), max(r[1] for r in res)
    print("over %d cases: delta %.3f units (E_NNI_BIG = %g), explicit neighbours %.3f units (E_EXPL_BIG = %g)"
          % (len(res), worst_n, E_NNI_BIG, worst_x, E_EXPL_BIG))
    assert E_NNI_BIG / 2 < worst_n <= E_NNI_BIG
    assert E_EXPL_BIG / 2 < worst_x <= E_EXPL_BIG
    assert NC.TOL_NNI_BIG == 8 * E_NNI_BIG * 2.0 ** -53 and TOL_EXPL_BIG == 8 * E_EXPL_BIG * 2.0 ** -53
    assert E_NNI_BIG > NC.E_NNI                                          # deep trees need the wider bound; small ones keep theirs


# ---- the move sample --------------------------------------------------------------------------------------------------------------
def node_depths(child):
    R = child.shape[0]
    N = R + 1
    depth = np.zeros(R, dtype=np.int64)
    for i in range(R - 1, -1, -1):
        for ch in child[i]:
            if ch >= N:
                depth[ch - N] = depth[i] + 1
    return depth


@pytest.mark.parametrize("name", list(EC.BIG))
def test_move_sample(name):
    _, child, _, _ = EC.big_case(name)
    for c in child:
        R = c.shape[0]
        moves = nni_moves(c)
        pick = NC.move_sample(c)
        assert pick == NC.move_sample(c.copy(), k=24) and pick == sorted(set(pick))
        assert len(pick) == 24 and set(pick) <= set(moves)
        deepest = int(np.argmax(node_depths(c)))
        for r in (0, R - 2, deepest):
            assert (r, 0) in pick and (r, 1) in pick
        assert ((R - 1, 0) in pick) == ((R - 1, 0) in moves) and ((R - 1, 1) in pick) == ((R - 1, 1) in moves)
        rows = np.array(sorted({r for r, _ in pick}))
        assert np.diff(rows).max() <= R / 4                              # spread over the rows: 16 evenly spaced moves lie R / 8 rows apart
    small = np.array([[0, 1], [3, 2]], dtype=np.int32)
    assert NC.move_sample(small) == nni_moves(small)


# ---- the cases: what the device test takes for granted -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement on scipy's matrices over the whole case: loglik [5], delta, absd [5][N-1][2], L [5][S]"""
    g, child, blen, Q = EC.big_case(name)
    res = [NR.tree_nni(c, m, PRIOR, g, want_sites=True) for c, m in zip(child, branch_matrices(Q, blen))]
    out = tuple(np.array([r[k] for r in res]) for k in range(4))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(EC.BIG))
def test_many_taxa_cases(name):
    kw = EC.BIG[name]
    g, child, blen, Q = EC.big_case(name)
    ll, delta, absd, L = restated(name)
    print("%s: site factors in [%.3g, %.3g], %d -inf, %d NaN" % (name, L.min(), L.max(), np.isneginf(delta).sum(), np.isnan(delta).sum()))
    assert (L >= ROOMY).all() and np.isfinite(L).all() and np.isfinite(ll).all()
    miss = missing_moves(child)
    np.testing.assert_array_equal(np.isnan(delta), miss)
    assert (np.isfinite(delta) | np.isneginf(delta))[~miss].all()
    assert not miss[:, :-1].any()
    if kw['shape'] == 'balanced':
        assert not np.isneginf(delta).any() and not miss.any() and np.isfinite(delta[:, -1]).all()
    elif kw['shape'] == 'caterpillar' or name == 'random-N512':          # (the random trees of 129 and 257 taxa happen to have none)
        assert np.isneginf(delta).any()
    if kw['shape'] == 'caterpillar':
        assert miss[:, -1].all()                                         # a leaf at the root of every tree: no move across the root
    if name == 'caterpillar-N512':
        assert np.isneginf(delta).sum() == 55 and np.isnan(delta).sum() == 2 * 5


@pytest.mark.parametrize("name", [n for n, kw in EC.BIG.items() if kw['N'] in (129, 512) and kw['S'] == 65 and not kw.get('generic')])
def test_apply_nni_on_deep_trees(name):
    """the sampled neighbours as explicit trees: one clade changes (none when the move only shifts the root), and the restated
    log-likelihood of the neighbour is the restated loglik + delta within TOL_EXPL_BIG (S + sum |log L| + sum |log L'|)"""
    g, child, blen, Q = EC.big_case(name)
    ll, delta, _, L = restated(name)
    N, S = g.shape[0], g.shape[1]
    R = N - 1
    worst, seen, dead = 0.0, 0, 0
    for t in (0, child.shape[0] - 1):                                    # the generating tree and its last neighbour
        M = branch_matrices(Q, blen[t])
        base = NC.clades(child[t])
        root_kids = {int(child[t][R - 1, 0]), int(child[t][R - 1, 1])}
        a0 = np.abs(np.log(L[t])).sum()
        memo = {}
        for row, side in NC.move_sample(child[t]):
            c2, b2 = apply_nni(child[t], blen[t], row, side)
            new = NC.clades(c2)
            changed = 0 if (row < R - 1 and N + row in root_kids) else 1
            assert len(base - new) == changed and len(new - base) == changed, (t, row, side)
            ll2, a2 = NC.restated_loglik(c2, NC.matrices_of(b2, blen[t], M), PRIOR, g, memo)
            lhs = ll[t] + delta[t, row, side]
            seen += 1
            if np.isneginf(lhs) or np.isneginf(ll2):
                assert lhs == ll2, (t, row, side)
                dead += 1
                continue
            err = abs(lhs - ll2) / (S + a0 + a2)
            worst = max(worst, err)
            assert err <= TOL_EXPL_BIG, (t, row, side, lhs, ll2, err)
    print("%s: worst |(loglik + delta) - loglik of the neighbour| / (S + sum |log L| + sum |log L'|) = %.3g (TOL_EXPL_BIG %.3g) over %d "
          "moves, %d impossible" % (name, worst, TOL_EXPL_BIG, seen, dead))


def test_strided_sets_stay_clear_of_the_floor():
    sample = [0, 1, 2, 64, 127, 128, 129, 130]
    for mixed in (False, True):
        g, child, blen, Q = EC.large_strided(mixed)
        for t in (sample[1], sample[-1]):
            ll, delta, _, L = NR.tree_nni(child[t], branch_matrices(Q, blen[t]), PRIOR, g, want_sites=True)
            assert (L >= ROOMY).all() and np.isfinite(ll)
            np.testing.assert_array_equal(np.isnan(delta), missing_moves(child[t:t + 1])[0])
        for w in range(128, 131):
            assert (child[w].tobytes() != child[w - 128].tobytes()) == mixed
    for cus in (64, 256, 304):
        cap = EC.updown_cap(5, cus)
        T = EC.strided_T(5, 3, cus)
        g, child, blen, Q = EC.small_mixed(T, cap)
        for w in range(cap, 3 * T):                                      # one workgroup's successive items: another row order
            assert child[w // 3].tobytes() != child[(w - cap) // 3].tobytes()
    L = TR.trees_site_factors(child, branch_matrices(Q, blen), PRIOR, g)
    assert (L >= ROOMY).all() and (g.sum(axis=2) == 4).any()


# ---- the floor of the range ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scaled():
    g, child, blen, Q = EC.scaled_base()
    M = branch_matrices(Q, blen)                                         # fixed: the scaled alignments see the same matrices
    return g, child, M, TR.trees_site_factors(child, M, PRIOR, g), NR.trees_nni(child, M, PRIOR, g)


@pytest.mark.parametrize("place", EC.PLACES)
def test_reference_on_the_scaled_cases(place, scaled):
    """what test_gpu_treenni_edges.py asks of the device, asked of the restatement first.  2^-900 and inside: every entry keeps
    the bits it has on the unscaled alignment (the scaling is by exact powers of two and nothing underflows).  at-the-floor: a
    neighbour's own factor may be subnormal beside a tree's factor in [2^-1020, 2^-1019), so only the pattern and 1e-6 are
    claimed (measured: 98 of 110 entries keep their bits, the others move by at most 1.5e-14).  Below the floor: NaN everywhere."""
    g, child, M, L0, (ll0, delta0, absd0) = scaled
    assert np.isfinite(ll0).all() and (L0 > 2.0 ** -200).all()
    miss = missing_moves(child)
    np.testing.assert_array_equal(np.isnan(delta0), miss)
    e = EC.scaled_exponents(place, L0)
    gs = EC.scaled_leaves(g, e)
    at = list(EC.SCALED_SITES)
    L = TR.trees_site_factors(child, M, PRIOR, gs)
    ll, delta, _ = NR.trees_nni(child, M, PRIOR, gs)
    print(place, "scaled site factors in [%.3g, %.3g]" % (L[:, at].min(), L[:, at].max()))
    if place in ('2^-900', 'inside'):
        assert (L[:, at] >= FLOOR).all()
        np.testing.assert_array_equal(bits(delta), bits(delta0))
    elif place == 'at-the-floor':
        assert (L[:, at] >= FLOOR).all() and (L[:, at].min(axis=0) < 2.0 ** -1019).all()
        np.testing.assert_array_equal(np.isnan(delta), miss)
        np.testing.assert_array_equal(np.isneginf(delta), np.isneginf(delta0))
        same = bits(delta) == bits(delta0)
        fin = np.isfinite(delta0)
        print(place, "%d of %d entries keep their bits, the others move by at most %.3g"
              % (same.sum(), same.size, np.abs(delta[fin] - delta0[fin]).max()))
        np.testing.assert_allclose(delta[fin], delta0[fin], rtol=1e-6, atol=1e-6)
    else:
        assert (L[:, at] < FLOOR).all() and np.isnan(delta).all()
        if place == 'zero':
            assert (ll == -np.inf).all()
        else:
            assert np.isfinite(ll).all()


def test_random_columns_300_and_310_taxa():
    g, child, blen, Q = EC.random_columns(300)
    M = branch_matrices(Q, blen)
    L = TR.trees_site_factors(child, M, PRIOR, g)
    ll, delta, _ = NR.trees_nni(child, M, PRIOR, g)
    assert (L >= FLOOR).all() and L.min() < 1e-300 and np.isfinite(ll).all()
    np.testing.assert_array_equal(np.isnan(delta), missing_moves(child))     # no NaN beyond the moves that do not exist
    g, child, blen, Q = EC.random_columns(310)
    M = branch_matrices(Q, blen)
    L = TR.trees_site_factors(child, M, PRIOR, g)
    ll, delta, _ = NR.trees_nni(child, M, PRIOR, g)
    out = (L < FLOOR).any(axis=1)
    assert out[0] and (L[0] > 0).all() and np.isfinite(ll[0]) and np.isnan(delta[0]).all()
    assert np.isnan(delta[out]).all()
