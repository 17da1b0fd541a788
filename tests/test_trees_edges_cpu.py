"""The edges of scored tree sets without a GPU (DESIGN.md sections 11 and 13): the preconditions of every case of
trees_edges_cases.py, read from the NumPy restatement alone (scipy's expm); the schedule depths of 129 to 512 taxa; the
restatement at the floor of the double range against the same formulas at 50 digits (E_REF_FLOOR) and on the scaled cases the
device is asked afterwards; what optimize_branches does with a gradient that is not finite.

Every test here fails on import without treegrad_ref.FLOOR and phylo_amd.treeopt.OutOfRangeError."""
import numpy as np
import pytest

import treegrad_ref as TR
import trees_edges_cases as EC
from phylo_amd import _ffi
from phylo_amd.treeopt import OutOfRangeError, optimize_branches
from test_treegrad_cpu import gapped
from treegrad_cases import E_REF, E_REF_FLOOR, TOL, branch_matrices
from trees_edges_cases import FLOOR, PRIOR, ROOMY


def factors(g, child, blen, Q):
    return TR.trees_site_factors(child, branch_matrices(Q, blen), PRIOR, g)


# ---- A. 129 to 512 taxa --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.BIG))
def test_many_taxa_cases_stay_clear_of_the_floor(name):
    kw = EC.BIG[name]
    g, child, blen, Q = EC.big_case(name)
    N = kw['N']
    assert g.shape == (N, kw['S'], 4) and child.shape == (5, N - 1, 2)
    assert len({c.tobytes() for c in child}) == 5                        # the generating tree and four different neighbours
    assert all((b[:, 1] == 0).any() and (b[:, 0] > 0).all() for b in blen)   # zero-length right-hand branches in every tree
    coded = (((g == 0) | (g == 1)).all(axis=2) & (g.sum(axis=2) >= 1)).all()
    assert coded == (not kw.get('generic'))
    L = factors(g, child, blen, Q)
    print("%s: site factors in [%.3g, %.3g]" % (name, L.min(), L.max()))
    assert (L >= ROOMY).all() and np.isfinite(L).all()


def test_schedule_depths():
    """A stack of d slots needs 2^d leaves (section 11: need(root) <= floor(log2 N)), so 512 taxa reach 9 slots and PT2_MAX_DEPTH =
    10 is reached by no tree a context accepts: balanced trees of 257 and 512 taxa schedule at 8 and 9, past the 7 of the 128
    taxa the other suites stop at; a caterpillar at 1 and its neighbours within 2 (four site steps per pass); and pt2_unroll's
    two forms both occur among the cases."""
    deepest = {}
    for name, kw in EC.BIG.items():
        _, child, blen, _ = EC.big_case(name)
        depths = [_ffi.debug_tree_schedule(c, b)[1] for c, b in zip(child, blen)]
        assert depths == [EC.su_depth(c) for c in child], name
        assert max(depths) <= int(np.log2(kw['N']))
        deepest[name] = (depths[0], max(depths))
    assert deepest['balanced-N129'][0] == 7 and deepest['balanced-N257'][0] == 8 and deepest['balanced-N512'][0] == 9
    assert deepest['balanced-N512-S130-tile64'][0] == 9 and deepest['generic-balanced-N512'][0] == 9
    for N in (129, 257, 512):
        assert deepest['caterpillar-N%d' % N][0] == 1 and deepest['caterpillar-N%d' % N][1] <= 2       # U = 4
        assert deepest['random-N%d' % N][0] >= 3                                                       # U = 2


# ---- B. more items than workgroups -----------------------------------------------------------------------------------------------
def test_strided_sets():
    assert EC.updown_cap(512, 256) == 128 and EC.updown_cap(5, 256) == 2048 and EC.updown_cap(5, 64) == 512
    for cus in (1, 8, 64, 104, 120, 256, 304):
        cap = EC.updown_cap(5, cus)
        T = EC.strided_T(5, 3, cus)
        assert 3 * T >= cap + 5 and (3 * T) % cap and 3 * (T - 1) < cap + 5 + 3 * 2
        _, child, _, _ = EC.small_mixed(T, cap)
        for w in range(cap, 3 * T):                                      # one workgroup's successive items: another topology
            assert child[w // 3].tobytes() != child[(w - cap) // 3].tobytes()
    for mixed in (False, True):
        g, child, blen, Q = EC.large_strided(mixed)
        assert child.shape[0] == 131 > EC.updown_cap(512, 256)
        for t in (128, 129, 130):
            assert (child[t].tobytes() != child[t - 128].tobytes()) == mixed
        pick = [0, 128, 130]
        L = factors(g, child[pick], blen[pick], Q)
        assert (L >= ROOMY).all()
    g, child, blen, Q = EC.small_strided(40)
    assert (factors(g, child, blen, Q) >= ROOMY).all() and (g.sum(axis=2) == 4).any()


# ---- C. the restatement at the floor ---------------------------------------------------------------------------------------------
def test_reference_against_mpmath_at_the_floor():
    """The cases of test_treegrad_cpu.py::test_reference_against_mpmath (N = 5, S = 8, 20 trees, GTR-like and JC69, gaps),
    every site scaled through two leaves so that its factor lands in [2^-1020, 2^-1000] -- the exponent
    drawn per site, the first site of every tree at the floor itself, [2^-1020, 2^-1019).  The restatement against the same
    formulas at 50 digits on the SCALED rows, in units of (scale + |value|) 2^-53: terms of a site's L' and outer partials far
    smaller than L are subnormal there and lose bits, so this measures what the floor costs.  Measured: see E_REF_FLOOR
    (treegrad_cases.py).  At or below E_REF the bound 2^-1020 stands as the sweep's reverse pass states it (section 4b)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    mpf = mp.mpf
    from oracle import cpu_ref as O
    from trees_cases import random_rows
    N, S = 5, 8
    worst = 0.0
    for seed in range(20):
        for jc in (False, True):
            rng = np.random.default_rng(seed)
            g = gapped(N, S, rng)
            Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
            child, blen = random_rows(N, rng)
            M = branch_matrices(Q, blen)
            L0 = TR.site_factors(child, M, PRIOR, g)
            assert (L0 > 1e-30).all()
            target = np.concatenate([[1019], rng.integers(1000, 1020, size=S - 1)])      # L lands in [2^-(target+1), 2^-target)
            e = np.frexp(L0)[1] + target
            a, b = rng.choice(N, 2, replace=False)
            g[a] = np.ldexp(g[a], -(e // 2)[:, None])
            g[b] = np.ldexp(g[b], -(e - e // 2)[:, None])
            L = TR.site_factors(child, M, PRIOR, g)
            assert (L >= FLOOR).all() and (L <= ROOMY).all() and L[0] < 2.0 ** -1019
            _, grad, curv, scale = TR.tree_grad(child, M, Q, PRIOR, g)
            assert np.isfinite(grad).all() and np.isfinite(curv).all()
            Mm = [[[[mpf(float(v)) for v in r] for r in M[i, sd]] for sd in range(2)] for i in range(N - 1)]
            Qm = [[mpf(float(v)) for v in r] for r in Q]
            pm = [mpf(float(v)) for v in PRIOR]
            G = [[mpf(0), mpf(0)] for _ in range(N - 1)]
            Cv = [[mpf(0), mpf(0)] for _ in range(N - 1)]
            for s in range(S):
                rows = [[mpf(float(v)) for v in g[i, s]] for i in range(N)]
                Ls, d1, d2 = TR.site_terms(child.tolist(), Mm, Qm, pm, rows, mpf(0))
                for i in range(N - 1):
                    for sd in range(2):
                        G[i][sd] += d1[i][sd] / Ls
                        Cv[i][sd] += d2[i][sd] / Ls - (d1[i][sd] / Ls) ** 2
            for i in range(N - 1):
                for sd in range(2):
                    for val, exact in ((grad[i, sd], G[i][sd]), (curv[i, sd], Cv[i][sd])):
                        unit = (mpf(float(scale[i, sd])) + abs(exact)) * mpf(2) ** -53
                        worst = max(worst, float(abs(mpf(float(val)) - exact) / unit))
    print("reference against 50 digits at the floor: worst error %.3f units of (scale + |value|) 2^-53 (E_REF_FLOOR = %g, E_REF = %g)"
          % (worst, E_REF_FLOOR, E_REF))
    assert E_REF_FLOOR / 2 <= worst <= E_REF_FLOOR <= E_REF


@pytest.fixture(scope="module")
def scaled():
    g, child, blen, Q = EC.scaled_base()
    M = branch_matrices(Q, blen)
    return g, child, blen, Q, M, TR.trees_site_factors(child, M, PRIOR, g), TR.trees_grad(child, M, Q, PRIOR, g)


@pytest.mark.parametrize("place", EC.PLACES)
def test_reference_on_the_scaled_cases(place, scaled):
    """what test_gpu_trees_edges.py asks of the device, asked of the restatement first"""
    g, child, blen, Q, M, L0, (ll0, grad0, curv0, scale0) = scaled
    assert np.isfinite(ll0).all() and (L0 > 2.0 ** -200).all()
    e = EC.scaled_exponents(place, L0)
    gs = EC.scaled_leaves(g, e)
    sites = list(EC.SCALED_SITES)
    assert (np.delete(gs, sites, axis=1) == np.delete(g, sites, axis=1)).all()
    L = TR.trees_site_factors(child, M, PRIOR, gs)
    ll, grad, curv, scale = TR.trees_grad(child, M, Q, PRIOR, gs)
    want = np.ldexp(L0[:, sites], -e[None, :])
    print(place, "scaled site factors in [%.3g, %.3g]" % (L[:, sites].min(), L[:, sites].max()))
    if place == '2^-900':
        np.testing.assert_array_equal(L[:, sites], want)
        np.testing.assert_array_equal(grad, grad0)
        np.testing.assert_array_equal(curv, curv0)
        np.testing.assert_allclose(ll, ll0 - e.sum() * np.log(2.0), rtol=1e-12, atol=0)
    elif place in EC.IN_RANGE:
        assert (L[:, sites] >= FLOOR).all() and (L[:, sites] <= ROOMY).all()
        if place == 'at-the-floor':
            assert (L[:, sites].min(axis=0) < 2.0 ** -1019).all()
        np.testing.assert_allclose(L[:, sites], want, rtol=2.0 ** -50, atol=0)
        assert np.isfinite(ll).all() and np.isfinite(grad).all() and np.isfinite(curv).all()
        for got, ref in ((grad, grad0), (curv, curv0)):
            err = np.abs(got - ref) / (scale0 + np.abs(ref))
            print(place, "worst |scaled - unscaled| / (scale + |value|) = %.3g (TOL %.3g)" % (err.max(), TOL))
            assert (err <= TOL).all()
    else:
        assert (L[:, sites] < FLOOR).all()
        assert np.isnan(grad).all() and np.isnan(curv).all()
        if place == 'just-below':
            assert (L[:, sites].max(axis=0) >= 2.0 ** -1021).all()
        if place == 'zero':
            assert (L[:, sites] == 0).all() and (ll == -np.inf).all()
        else:
            assert (L[:, sites] > 0).all() and np.isfinite(ll).all()       # (a subnormal factor is rounded: no prediction of ll)


def test_random_columns_reach_the_floor_between_300_and_310_taxa():
    g, child, blen, Q = EC.random_columns(300)
    L = factors(g, child, blen, Q)
    print("N = 300: smallest site factor per tree", L.min(axis=1))
    assert (L >= FLOOR).all() and L[0].min() == pytest.approx(2.7e-304, rel=0.05)
    ll, grad, curv, _ = TR.trees_grad(child, branch_matrices(Q, blen), Q, PRIOR, g)
    assert np.isfinite(ll).all() and np.isfinite(grad).all() and np.isfinite(curv).all()
    g, child, blen, Q = EC.random_columns(310)
    L = factors(g, child, blen, Q)
    print("N = 310: smallest site factor per tree", L.min(axis=1), "below the floor", (L < FLOOR).sum(axis=1))
    assert ((L[0] < 2.0 ** -1022).sum(), (L[0] == 0).sum()) == (11, 0)
    ll, grad, curv, _ = TR.trees_grad(child, branch_matrices(Q, blen), Q, PRIOR, g)
    # trees 0 and 1: a finite loglik beside factors below the floor -- what the rule is for; tree 2 has a factor that IS zero and
    # loglik -inf (the older NaN rule covers it); none of the three stays in range
    out = (L < FLOOR).any(axis=1)
    assert out.tolist() == [True, True, True] and np.isfinite(ll).tolist() == [True, True, False] and ll[2] == -np.inf
    assert np.isnan(grad).all() and np.isnan(curv).all()


# ---- C. the optimiser ------------------------------------------------------------------------------------------------------------
def stub(bad_at_start=(), bad_beyond=None):
    """a concave toy function of T trees; tree t in bad_at_start has a NaN gradient beside a finite value everywhere; with
    bad_beyond, a tree's derivatives are NaN wherever its first length exceeds it -- the value stays finite and keeps rising"""
    target = 0.7

    def fn(b):
        ll = -((b - target) ** 2).sum(axis=(1, 2))
        g, c = -2 * (b - target), np.full(b.shape, -2.0)
        for t in bad_at_start:
            g[t], c[t] = np.nan, np.nan
        if bad_beyond is not None:
            out = b[:, 0, 0] > bad_beyond
            g[out], c[out] = np.nan, np.nan
        return ll, g, c

    return fn


def test_optimizer_refuses_a_start_without_a_gradient():
    b = np.full((3, 2, 2), 0.5)
    with pytest.raises(OutOfRangeError, match=r"gradient of tree 1 is not finite") as e:
        optimize_branches(stub(bad_at_start=(1,)), None, b)
    assert isinstance(e.value, ValueError) and '2^-1020' in str(e.value)

    def inf_ll(x):
        ll, g, c = stub()(x)
        ll[2] = -np.inf
        return ll, g, c

    with pytest.raises(OutOfRangeError, match=r"log-likelihood of tree 2 is not finite"):
        optimize_branches(inf_ll, None, b)
    out = optimize_branches(stub(), None, b)
    assert out['converged'].all()


def test_optimizer_refuses_a_trial_without_a_gradient():
    """the full Newton step from 0.5 lands on 0.7 = beyond 0.6: refused although the value rises; the halved step (0.6) is taken,
    and the tree never holds a point whose gradient is not finite"""
    b = np.full((2, 2, 2), 0.5)
    seen = []

    def fn(x):
        seen.append(x.copy())
        return stub(bad_beyond=0.6)(x)

    out = optimize_branches(fn, None, b, max_iter=12)
    assert len(seen) > 2 and (seen[1][:, 0, 0] > 0.6).all()              # the first trial was out of range ...
    assert (out['history'][1] == out['history'][0]).all()                # ... and refused: the trees kept their lengths
    assert (out['history'][2] > out['history'][1]).all()                 # the halved step was accepted
    assert np.isfinite(out['grad']).all() and np.isfinite(out['loglik']).all()
    assert (out['blen'][:, 0, 0] <= 0.6).all()
    assert (np.diff(out['history'], axis=0) >= 0).all()
    np.testing.assert_allclose(out['blen'], 0.6, rtol=1e-12)            # every later trial crosses the edge: none is taken
    assert not out['converged'].any()


def test_runner_reports_an_out_of_range_tree(monkeypatch, capsys):
    import os
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, root)
    try:
        import runner
    finally:
        sys.path.remove(root)
    import phylo_amd.datasets
    import phylo_amd.vcsmc

    class Stub:
        def __init__(self, *a, **k):
            pass

        def train(self, **k):
            raise OutOfRangeError("optimize_branches: the gradient of tree 4 is not finite at the starting lengths")

    monkeypatch.setattr(phylo_amd.vcsmc, 'VCSMC', Stub)
    monkeypatch.setattr(phylo_amd.datasets, 'load_dataset', lambda *a, **k: {})
    with pytest.raises(SystemExit) as e:
        runner.main(['--dataset', 'primate_data_wang', '--score_trees', 'x.nwk', '--score_opt', 'true'])
    assert 'runner.py --score_opt' in str(e.value.code) and 'tree 4' in str(e.value.code) and 'x.nwk' in str(e.value.code)
