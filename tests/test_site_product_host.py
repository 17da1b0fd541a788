"""The site-product contract at the edges of the double range, without a GPU.

1. The pair update pm_lp_mul2 (what the merge kernels run) against the per-factor update pm_lp_mul (the contract's statement),
   both through the host body of phylo_debug_site_product, against the C oracle's per-factor update and against a restatement in
   Python (tests/site_product_ref.py): every bit of p', E' and extra', on 2 * 10^6 random triples, the boundary grid and products
   steered onto 2^-1022, 2^-1021 and 2^1024.  Every branch of the pair form is counted from the inputs.
2. The C oracle's row sum -- the reference the GPU is compared with bit for bit -- against mpmath at 60 digits."""
import math

import mpmath as mp
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from tests import site_product_cases as SC
from tests import site_product_ref as R

PI = np.full((1, 4), 0.25)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bit_equal(a, b, what=""):
    """the rule of tests/test_gpu_parity.py: every bit, NaN payloads aside"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    bad = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), "%s: %d of %d values differ; first at %d: %r against %r" % (
        what, bad.sum(), bad.size, np.flatnonzero(bad)[0], a[bad][:1], b[bad][:1])


def assert_same_state(got, want, what):
    assert_bit_equal(got[0], want[0], what + ": p'")
    np.testing.assert_array_equal(np.asarray(got[1], dtype=np.int64), np.asarray(want[1], dtype=np.int64), err_msg=what + ": E'")
    assert_bit_equal(got[2], want[2], what + ": extra'")


def oracle_log(x):
    """log of a factor that is not a positive normal number: the special values by rule, a subnormal by the oracle's log, which
    test_log_of_subnormal_factors_is_within_an_ulp holds against mpmath"""
    return CO.math_probe(1, np.atleast_1d(np.asarray(x, dtype=np.float64)))


def all_triples():
    gp, g1, g2 = R.boundary_grid()
    sp, s1, s2, _ = R.steered_triples()
    rp, r1, r2 = R.random_triples(2_000_000, seed=20)
    return np.concatenate([gp, sp, rp]), np.concatenate([g1, s1, r1]), np.concatenate([g2, s2, r2])


def test_log_of_subnormal_factors_is_within_an_ulp():
    """what `extra` receives for a subnormal factor: pm_log's 2^54 rescale.  Host bits = oracle bits, and within one ulp of the
    60-digit log; zero, negative, infinite and NaN factors by the rule of a sum of logs."""
    rng = np.random.default_rng(3)
    x = np.concatenate([[5e-324, 2.0 ** -1023, R.SUBMAX, 2.0 ** -1050], np.ldexp(1.0 + rng.random(2000), rng.integers(-1074, -1022, 2000))])
    got = oracle_log(x)
    host = _ffi.debug_site_product(np.ones(x.size), x, np.ones(x.size))['each'][2]      # extra' = 0.0 + log x
    assert_bit_equal(host, got, "log of a subnormal factor, host against oracle")
    with mp.workdps(60):
        for xi, gi in zip(x, got):
            assert abs(mp.mpf(float(gi)) - mp.log(mp.mpf(float(xi)))) <= float(np.spacing(abs(gi))), (xi, gi)
    sp = oracle_log([0.0, -0.0, math.inf, -1.0, -math.inf, -5e-324, math.nan])
    assert sp[0] == -math.inf and sp[1] == -math.inf and sp[2] == math.inf and np.isnan(sp[3:]).all()


def test_pair_update_is_the_per_factor_update_on_every_branch():
    p, x1, x2 = all_triples()
    br = R.branch_of(p, x1, x2)
    counts = {name: int((br == i).sum()) for i, name in enumerate(R.BRANCHES)}
    print("branches of the pair form:", counts)
    for name, n in counts.items():
        assert n > 0, "no triple takes the branch %r" % name
    host = _ffi.debug_site_product(p, x1, x2)
    assert_same_state(host['pair'], host['each'], "host pair form against host per-factor form")
    want = R.lp_two_np(p, x1, x2, oracle_log)
    assert_same_state(host['each'], want, "host per-factor form against the restatement")
    assert_same_state(CO.lp_probe(p, x1, x2), want, "oracle per-factor form against the restatement")
    # a kept pair changes p and E only; a mantissa stays in [1, 2)
    assert ((host['pair'][0] >= 1.0) & (host['pair'][0] < 2.0)).all()
    assert (host['pair'][2][br == 0] == 0.0).all()
    # the scalar restatement (math.frexp, Python integers) on the grid, the steered products and a slice of the random triples
    n_fixed = p.size - 2_000_000
    for i in list(range(n_fixed)) + list(range(n_fixed, p.size, 997)):
        sp, sE, sx = R.lp_two(float(p[i]), float(x1[i]), float(x2[i]), lambda v: float(oracle_log(v)[0]))
        assert sp == want[0][i] and sE == want[1][i], (i, p[i], x1[i], x2[i])
        assert sx == want[2][i] or (math.isnan(sx) and math.isnan(want[2][i])), (i, p[i], x1[i], x2[i])


def test_steered_products_sit_on_the_thresholds():
    """The inputs of the test above really walk the three thresholds: for each, products that are exactly on it, one ulp below, one
    ulp above, and inexact ones that ROUND UP onto it -- for 2^-1022 those were rounded on the subnormal grid, the reason the pair
    form keeps q only from 2^-1021 on; and among the rejected pairs some whose two per-factor updates give a mantissa that the
    product on the subnormal grid has lost."""
    p, x1, x2, target = R.steered_triples()
    with np.errstate(all='ignore'):
        q = (p * x1) * x2
    for t in (-1022, -1021, 1024):
        B = math.inf if t == 1024 else 2.0 ** t
        below = R.MAXF if t == 1024 else float(np.nextafter(B, 0.0))
        sel = np.flatnonzero(target == t)
        on = sel[q[sel] == B]
        assert on.size and (q[sel] == below).any(), t
        if t != 1024:
            assert (q[sel] == np.nextafter(B, 4.0)).any(), t
        exact = [R.exact_product(p[i], x1[i], x2[i]) for i in on]
        edge = R.Fraction(2) ** t
        assert any(e == edge for e in exact), t
        assert any(e < edge for e in exact), "no product rounds up onto 2^%d" % t
        if t == 1024:
            assert any(e > edge for e in exact)
    # q = 2^-1022 although 53-bit rounding of the mantissa product gives 2 - 2^-52: taking q would give p' = 1 one exponent up
    sel = np.flatnonzero((target == -1022) & (q == R.TINY))
    each = _ffi.debug_site_product(p[sel], x1[sel], x2[sel])['each']
    assert (each[0] == 2 - 2.0 ** -52).any() and (each[0] == 1.0).any()
    assert (each[1][each[0] == 2 - 2.0 ** -52] == -1023).all() and (each[1][each[0] == 1.0] == -1022).all()


# ---- 2. the oracle's row sum against 60-digit arithmetic -------------------------------------------------------------------------

SIZES = [1, 63, 64, 65, 129, 2047, 2048, 2049, 5000]


def family(name, S, rng):
    m = 1.0 + rng.random(S)
    if name == 'whole normal range':                 # 4 f must stay finite: exponents -1022 .. 1021
        return np.ldexp(m, rng.integers(-1022, 1022, S))
    if name == 'pairs under 2^-1021':
        return np.ldexp(m, rng.integers(-530, -504, S))
    if name == 'pairs over 2^1023':
        return np.ldexp(m, rng.integers(505, 521, S))
    if name == 'one in five subnormal':
        f = rng.uniform(0.01, 1.0, S)
        sub = rng.random(S) < 0.2
        f[sub] = np.ldexp(m[sub], rng.integers(-1074, -1023, int(sub.sum())))
        return f
    assert name == 'exponents +-600'
    return np.ldexp(m, rng.integers(-600, 601, S))


FAMILIES = [(n, S) for n in ('whole normal range', 'pairs under 2^-1021', 'pairs over 2^1023', 'one in five subnormal') for S in SIZES]
FAMILIES.append(('exponents +-600', 5000))


def oracle_row(f):
    """the oracle's canonical sum over sites of a row whose site likelihoods are exactly f: pi = 1/4 and rows (4 f, 0, 0, 0);
    scaling by a power of two is exact (subnormal f included: 4 f moves away from zero), 4 f is finite"""
    f = np.asarray(f, dtype=np.float64)
    core = np.zeros((1, 1, f.size, 4))
    with np.errstate(all='ignore'):
        core[0, 0, :, 0] = 4.0 * f
    assert np.isfinite(core[0, 0, np.isfinite(f), 0]).all()
    return float(CO.forest_loglik(PI, core, np.ones((1, 1), dtype=np.int32))[0])


@pytest.mark.parametrize("name,S", FAMILIES, ids=["%s-S%d" % (n.replace(' ', '_'), S) for n, S in FAMILIES])
def test_oracle_row_sum_against_mpmath(name, S):
    """|got - exact| <= u (S + a) + b u sum_c |v_c| (columns with subnormal factors: see the end), u = 2^-53, v_c the 64 * tiles column values (exact
    sums of logs of the column's factors; the computed ones differ from them by the bound itself, times u: nothing), derived from
    contract v5 alone, first order in u (the second-order terms are below S u times the bound, < 10^-12 of it, and sit in the
    `+ 1` of a):

      a = 4 * (non-empty columns, 64 * tiles for S >= 64 * tiles) + 1, per column:
        * the mantissa product: ONE rounding per factor, (1 + d)^n_c with |d| <= u, moves log(product) by <= n_c u; all columns: S u;
        * pm_log(p), p in [1, 2): within 1 ulp of a value below 0.7, <= u                                            -> 1 per column;
        * pm_lp_finish, ((log p + dE lo) + dE hi) + extra: two products and three adds, each rounded with relative error u of
          its own result.  |dE lo| < 10^-9 |dE hi|, |log p| < 0.7 and the last two sums are v_c up to what was just bounded, so
          the five results add up to at most 3 |v_c| + 3                                          -> 3 per column, and 3 in b;
        * hi + lo = ln 2 to 2^-102 relative, times |E| < 10^5: nothing                                        (the `+ 1`).
      b = 3 + 6 + (tiles - 1):
        * six levels of the adjacent-pair tree: each add is rounded relative to a partial sum, which is at most the sum of |v_c|
          below it; a level's partial sums together at most sum_c |v_c|                                                   -> 6;
        * tiles - 1 adds of tile values, each partial total at most sum_c |v_c|                                  -> tiles - 1.
      a column with m_c > 0 subnormal factors (they go through pm_log into `extra`, one add each): every intermediate of the
      column -- a partial sum of `extra`, v_c before `extra` is added, v_c -- is at most A_c = sum_s |log f_s| in magnitude, so A_c
      takes the place of |v_c| in the terms above; pm_log is within 1 ulp and ulp(y) <= 2 u |y|, so the subnormal factors' logs
      together are off by <= 2 u A_c; the m_c adds into `extra` are rounded relative to partial sums <= A_c     -> (b + 2 + m_c) A_c.

    Site tile 2048 (the default): S = 2049 and 5000 span two and three tiles."""
    rng = np.random.default_rng(1000 * len(name) + S)
    f = family(name, S, rng)
    T = CO.site_tile(S)
    assert T == 2048
    got = oracle_row(f)
    exact, bound = R.row_bound(f, T)
    err = float(abs(mp.mpf(got) - exact))
    print("%s S=%d: got %.17g |err| %.3g bound %.3g" % (name, S, got, err, bound))
    assert math.isfinite(got)
    assert err <= bound, (name, S, got, err, bound)
    # the family is what its name says: many of a column's adjacent factors leave the range together (S < 65 holds no pair)
    if S >= 129 and name.startswith('pairs'):
        br = R.branch_of(np.ones(S - 64), f[:-64], f[64:])
        assert (br == (3 if 'under' in name else 4)).mean() > 0.3


def test_oracle_row_sum_special_factors():
    """One special factor among ordinary ones gives what a sum of logs gives, wherever it sits: first and last site, either factor
    of a pair of steps, the last column, either side of the tile boundary."""
    rng = np.random.default_rng(8)
    for S in (1, 65, 130, 2049, 4100):
        base = rng.uniform(0.1, 1.0, S)
        for at in sorted({0, S - 1, min(63, S - 1), min(64, S - 1), min(127, S - 1), min(2047, S - 1), min(2048, S - 1)}):
            for v, want in ((0.0, -math.inf), (math.inf, math.inf), (math.nan, math.nan), (-1.0, math.nan)):
                f = base.copy()
                f[at] = v
                got = oracle_row(f)
                assert got == want or (math.isnan(want) and math.isnan(got)), (S, at, v, got)
            f = base.copy()
            f[at] = 5e-324
            got = oracle_row(f)
            exact, bound = R.row_bound(f, 2048)
            assert math.isfinite(got) and abs(mp.mpf(got) - exact) <= bound, (S, at, got)
    # 0 and +inf in one row: -inf + inf = NaN, in one column, in two columns of a tile, and in two tiles (either order)
    for S, i, j in ((130, 3, 67), (130, 3, 4), (4100, 10, 3000), (4100, 3000, 10), (4100, 2047, 2048)):
        f = rng.uniform(0.1, 1.0, S)
        f[i], f[j] = 0.0, math.inf
        assert math.isnan(oracle_row(f)), (S, i, j)


# ---- 3. the oracle reaches the classes the GPU cases are about ---------------------------------------------------------------------

@pytest.mark.parametrize("N,S,T,K,kinds,need", SC.SWEEP_CASES, ids=["S%d-T%d-%s" % (c[1], c[2], c[4]) for c in SC.SWEEP_CASES])
def test_oracle_sweeps_reach_the_intended_classes(N, S, T, K, kinds, need):
    """The inputs of tests/test_gpu_site_product_edges.py, on the CPU: the replay of the oracle's node rows finds every class the
    case names, and the weights go bad the way the case says."""
    g = SC.scaled_leaves(N, S, T or 2048, kinds, seed=1)
    assert np.isfinite(SC.site_likelihoods(g, PI)).all() == (kinds != SC.ALLBAD)        # leaves spoil a forest in that case only
    lam = np.full(N - 1, 10.0)
    CO.set_site_tile(T)
    try:
        ref = CO.sweep(g, O.get_Q(O.init_y_q()), PI, lam, lam, K, 3, want_nodes=True)
    finally:
        CO.set_site_tile(0)
    counts = SC.replay(SC.site_likelihoods(ref['nodes'], PI), T or 2048)
    for c in need:
        assert counts[c] > 0, (c, counts)
    x = SC.site_likelihoods(ref['nodes'], PI)
    if kinds == SC.SPECIAL and S == 449:                       # every kind of special factor, and weights of every kind
        assert (x < 0).any() and np.isnan(x).any() and np.isinf(x).any() and (x == 0).any() and ((x > 0) & (x < R.TINY)).any()
        ll = ref['log_likelihood']
        assert np.isnan(ll).any() and (ll == math.inf).any() and np.isfinite(ll).any()
        particles, lanes = SC.special_spread(x[N - 2])         # the last rank event: every particle, many lanes besides lane 7
        assert particles == K and len(set(lanes) - {7}) >= 2
    if kinds == SC.TILES:                                      # zeros and infinities decide results: nothing hides behind a NaN factor
        assert not (np.isnan(x) | (x < 0)).any()
        assert len(SC.rows_decided_by_the_tile_sum(x, T or 2048)) > 0      # a -inf tile, later a +inf tile, NaN by the tile sum alone
        ll = ref['log_likelihood']
        assert (ll == -math.inf).any() and (ll == math.inf).any() and np.isnan(ll).any() and np.isfinite(ll).any()


def test_oracle_coded_sweep_reaches_the_intended_classes():
    g = SC.coded_leaves(6, 200, seed=2)
    lam = np.full(5, 1e155)
    ref = CO.sweep(g, O.get_Q(O.init_y_q()), PI, lam, lam, 64, 3, want_nodes=True)
    counts = SC.replay(SC.site_likelihoods(ref['nodes'], PI), 2048)
    for c in SC.CODED_NEED:
        assert counts[c] > 0, (c, counts)
    assert counts['inf'] == 0                                  # not reachable through coded leaves: probabilities stay <= 1


def test_oracle_twisted_coded_jc69_prices_zero_code_pairs():
    """The look-ahead potential of two coded leaves is priced per code pair, sum_c count_c log f_c.  Under the JC69 closed form at
    rates of 1e155 every branch is shorter than 2^-54, 1/4 - 1/4 exp(-t) is exactly 0, so f_c = 0 for every mismatching pair of
    codes and count_c log 0 = -inf: at rank event 0, where all roots are leaves, every potential of every particle is -inf."""
    N, S, K = 6, 200, 48
    g = SC.coded_leaves(N, S, seed=2)
    lam = np.full(N - 1, 1e155)
    ref = CO.sweep_twisted(g, O.jc_Q(), PI, lam, lam, K, 1, 7, jc=True, want_potentials=True)
    P = CO.expm_batched(O.jc_Q(), ref['left_branches'][0], jc=True)
    assert (P == np.eye(4)).all()                              # f_c = pi_a [i == a] [j == a]: exactly 0 for i != j
    codes = g.argmax(axis=2)
    assert all((codes[i] != codes[j]).any() for i in range(N) for j in range(i))
    assert np.isneginf(ref['potentials'][0][:, :N * (N - 1) // 2]).all()
