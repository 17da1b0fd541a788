"""The two numerical schemes the reverse pass does NOT share with the oracle, each against a high-precision statement of the same
operation (inputs and references: tests/grad_schemes_ref.py):
  * the Frechet derivative of expm as a scaled Taylor series with pairwise squarings, in its one-lane form (pg_expm4_frechet, what
    pg_twist_finish runs) and its quad form (pg_expm4_frechet_row, what pg_node_finish runs), through phylo_debug_frechet;
  * the reciprocal of a site likelihood (pg_rcp: v_rcp_f64 and two Newton steps), through phylo_math_probe op 5.
The whole-gradient tests (tests/test_gpu_grad.py) compare sums over hundreds of nodes at 1e-9; here one matrix, one number at a time."""
import time

import numpy as np
import pytest

from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset
from tests import grad_schemes_ref as R

# max |L_gpu - L_ref| <= FRECHET_RTOL max |L_ref| per matrix, for ||A||_1 <= 4096.  The pass's contract is 1e-9 per gradient block and
# L enters d_Q linearly, so 1e-11 leaves two orders for everything else; the scheme itself in binary64 is good for ~3e-13 on this
# range (a NumPy transcription against mpmath), and reference B is within 1e-12 of reference A (asserted below, measured 6.9e-13).
# Measured on the device: 4e-16 at s = 0 rising with the squarings to 9.6e-13 at s = 13 against reference A, 3.4e-12 against B.
FRECHET_RTOL = 1e-11


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    genome = load_dataset('primate_data_wang')['genome'][:3, :16]
    with _ffi.Context(2, 3, 16) as c:
        c.set_leaves(genome)
        c.set_model(O.jc_Q(), np.full((1, 4), 0.25), np.full(2, 10.0), np.full(2, 10.0))
        yield c


@pytest.fixture(scope="module")
def grid():
    A, E, tags = R.grid_A()
    t0 = time.time()
    L = np.array([R.frechet_mpmath(a, e) for a, e in zip(A, E)])
    print('reference A: %d pairs at 60 digits in %.1f s' % (len(A), time.time() - t0))
    return A, E, tags, L


# ---- host only: reference B rests on reference A ----------------------------------------------------------------------------
def test_inputs_cover_every_class_and_scaling():
    for A in (R.grid_A()[0], R.batch_B()[0]):
        s, nt = R.plan(A)
        assert set(s.tolist()) == set(range(14)), sorted(set(s.tolist()))       # s = 0 .. 12, and 13 at ||A||_1 = 4096 itself
        assert set(nt.tolist()) == set(R.NTERMS)
        for sv in range(1, 14):                                                 # both classes that a scaled theta in (1/4, 1/2] can take
            assert set(nt[s == sv].tolist()) == {15, 18}, sv
    # the two sides of a boundary, one ulp of b apart, fall into different plans
    Q = R.generators()[1][1]
    for target, what in ((0.01, 1), (0.05, 1), (0.15, 1), (0.3, 1), (0.5, 0), (np.ldexp(0.3, 5), 1), (np.ldexp(0.5, 7), 0)):
        lo, hi = R.edge_b(Q, target)
        assert hi == np.nextafter(lo, np.inf)
        p = R.plan(np.array([R.a_of(Q, lo), R.a_of(Q, hi)]))
        assert p[what][0] != p[what][1], (target, p)


def test_scipy_frechet_agrees_with_mpmath_on_the_grid(grid):
    A, E, tags, LA = grid
    err = R.rel_err(R.frechet_scipy(A, E), LA)
    i = int(np.argmax(err))
    print('reference B against A: worst %.3g at %s' % (err[i], tags[i]))
    assert err[i] <= 1e-12, (err[i], tags[i])                                   # measured 6.9e-13 (JC-like Q, ||A||_1 = 4096)


# ---- the Frechet series on the device ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_frechet_series_against_mpmath(ctx, grid, form):
    A, E, tags, LA = grid
    L = ctx.frechet_probe(A, E, form)
    assert np.all(np.isfinite(L))
    err = R.rel_err(L, LA)
    i = int(np.argmax(err))
    s, nt = R.plan(A)
    print('form %d against reference A: worst %.3g at %s (s = %d, %d terms)' % (form, err[i], tags[i], s[i], nt[i]))
    for sv in sorted(set(s.tolist())):
        print('   s = %2d: worst %.3g' % (sv, err[s == sv].max()))
    assert err[i] <= FRECHET_RTOL, (err[i], tags[i])


@pytest.mark.gpu
def test_frechet_series_batch_layouts_and_forms_bit_identical(ctx):
    """The 20 037 pairs of reference B in three layouts -- as generated, sorted by norm (neighbours alike), shuffled so that
    neighbouring lanes (form 0) and neighbouring quads (form 1) differ in the number of squarings and in the term class -- and in
    ragged sub-batches: every matrix's result is the same bits wherever it stands and in both forms (form 1 is, element by element,
    the arithmetic of form 0), which a quad broadcast taken from a lane that has left the squaring loop would break; and every
    result is within FRECHET_RTOL of scipy.linalg.expm_frechet."""
    A, E = R.batch_B()
    n = len(A)
    s, nt = R.plan(A)
    t0 = time.time()
    ref = R.frechet_scipy(A, E)
    t_ref = time.time() - t0
    base = ctx.frechet_probe(A, E, 0)
    assert np.all(np.isfinite(base))
    by_norm = np.argsort(R.norm1_device(A), kind='stable')
    shuffled = R.shuffled_layout(s, nt)
    sp, ntp = s[shuffled], nt[shuffled]
    assert np.mean(sp[1:] != sp[:-1]) >= 0.95 and np.mean(ntp[1:] != ntp[:-1]) >= 0.5
    for form in (0, 1):
        for what, perm in (('as generated', np.arange(n)), ('sorted by norm', by_norm), ('shuffled', shuffled)):
            L = ctx.frechet_probe(A[perm], E[perm], form)
            bad = np.nonzero(np.any(bits(L).reshape(n, 16) != bits(base[perm]).reshape(n, 16), axis=1))[0]
            assert bad.size == 0, "form %d, %s: %d of %d matrices differ from form 0 as generated; first at %d (s = %d, %d terms)" % (
                form, what, bad.size, n, bad[0], s[perm][bad[0]], nt[perm][bad[0]])
        for m in (1, 3, 63, 64, 65, 257):                                       # ragged last wave / workgroup, a single quad
            L = ctx.frechet_probe(A[shuffled[:m]], E[shuffled[:m]], form)
            assert np.array_equal(bits(L), bits(base[shuffled[:m]])), (form, m)
    err = R.rel_err(base, ref)
    i = int(np.argmax(err))
    print('against reference B (%d pairs, %.1f s of scipy): worst %.3g (||A||_1 = %.6g, s = %d, %d terms)' % (
        n, t_ref, err[i], R.norm1_device(A[i:i + 1])[0], s[i], nt[i]))
    for sv in sorted(set(s.tolist())):
        print('   s = %2d: worst %.3g' % (sv, err[s == sv].max()))
    assert err[i] <= FRECHET_RTOL, (err[i], A[i], E[i])


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_frechet_series_identities(ctx, form):
    """A = 0: L = E as values (the series adds E to +0.0 and then zeros: a zero of E may come back with the other sign, nothing else
    changes).  Linear in E: E scaled by 2^-500 or 2^500 scales L by exactly that; E = 0 gives L = 0."""
    rng = np.random.default_rng(3)
    E = np.array([R.special_E(rng, k % 5) for k in range(40)])
    L = ctx.frechet_probe(np.zeros_like(E), E, form)
    assert np.array_equal(L, E)
    A, E, _ = R.grid_A()
    L = ctx.frechet_probe(A, E, form)
    zero = np.all(E == 0.0, axis=(1, 2))
    assert zero.any() and np.all(L[zero] == 0.0)
    ok = (np.max(np.abs(E), axis=(1, 2)) < 1e100) & (np.max(np.abs(E), axis=(1, 2)) > 1e-100)
    for p in (-500, 500):
        Ls = ctx.frechet_probe(A[ok], np.ldexp(E[ok], p), form)
        assert np.array_equal(bits(Ls), bits(np.ldexp(L[ok], p))), p


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_frechet_series_finite_for_generators_up_to_2_to_40(ctx, form):
    """Beyond ||A||_1 = 4096 nothing is asserted but finiteness, for generator matrices up to 2^40 (41 squarings of a matrix whose
    entries stay in [0, 1]).  The code caps the scaling at s = 60: from ||A||_1 > 2^59 on, theta exceeds 1/2 and 18 terms no longer
    converge, so the result is meaningless there -- a branch length of 1e17 expected substitutions, which no sweep produces."""
    rng = np.random.default_rng(4)
    As, Es = [], []
    for _, Q in R.generators():
        nq = R.norm1_device(R.a_of(Q, 1.0))[0]
        for norm in np.exp(rng.uniform(np.log(4096.0), np.log(2.0 ** 40), 40)).tolist() + [2.0 ** 40]:
            As.append(R.a_of(Q, norm / nq))
            Es.append(rng.normal(size=(4, 4)))
    A, E = np.array(As), np.array(Es)
    assert R.plan(A)[0].max() == 41
    assert np.all(np.isfinite(ctx.frechet_probe(A, E, form)))


# ---- the reciprocal ----------------------------------------------------------------------------------------------------------
def _ulps(got, want):
    return np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64))


@pytest.mark.gpu
def test_reciprocal_within_two_ulp_on_its_domain(ctx):
    """pg_rcp(x) against the correctly rounded 1.0 / x for normal x in [2^-1020, 2^1020].

    Outside the documented domain nothing is asserted; the device returns (MI355X, this test prints them):
      +0, -0, subnormal x (5e-324, 2^-1030), +inf, NaN -> NaN   (v_rcp_f64 gives inf or 0 and the Newton step forms 0 * inf);
      2^-1022 -> 2^1022 and 2^1022 -> 2^-1022 exactly; 2^1023 -> 2^-1023 and 1.7e308 -> 5.88e-309 (subnormal results, correct);
      negative normal x is as good as positive (-1 -> -1).
    No caller reaches the NaN cases with a finite log Z: pg_rcp only ever sees site likelihoods pi . x, a likelihood of 0 already
    makes the forward sweep's log Z -inf, and the smallest likelihood of a primate sweep is 4e-13 (the next test) -- a subnormal
    one needs hundreds of taxa without rescaling, which the forward sweep does not support either."""
    rng = np.random.default_rng(5)
    x = np.ldexp(rng.uniform(1.0, 2.0, 200000), rng.integers(-1020, 1020, 200000))
    worst = int(_ulps(ctx.math_probe(5, x), 1.0 / x).max())
    # around every power of two of a coarse ladder: 2^k (1 +- j ulp), j = 0 .. 4 (1/x crosses a binade there), and 1 +- j ulp
    k = np.arange(-1020, 1021, 17)
    near = [np.ldexp(1.0, k)]
    for j in range(1, 5):
        up, dn = np.ldexp(1.0, k), np.ldexp(1.0, k)
        for _ in range(j):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, 0.0)
        near += [up, dn]
    one = np.float64(1.0)
    around_one = [one]
    up = dn = one
    for _ in range(64):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, 0.0)
        around_one += [up, dn]
    x2 = np.concatenate(near + [np.array(around_one)])
    x2 = x2[(x2 >= 2.0 ** -1020) & (x2 <= 2.0 ** 1020)]
    worst_edges = int(_ulps(ctx.math_probe(5, x2), 1.0 / x2).max())
    print('pg_rcp: worst %d ulp on %d log-uniform x, %d ulp on %d x around powers of two' % (worst, x.size, worst_edges, x2.size))
    assert max(worst, worst_edges) <= 2            # worst seen: 0 ulp log-uniform, 1 ulp at the edges (with one Newton step: 10 and 14)
    probe = np.array([0.0, 5e-324, 2.0 ** -1030, 2.0 ** -1022, 2.0 ** 1022, 2.0 ** 1023, 1.7e308, np.inf, np.nan, -1.0, -0.0])
    print('pg_rcp outside its domain: ' + ', '.join('%r -> %r' % (float(a), float(b)) for a, b in zip(probe, ctx.math_probe(5, probe))))


@pytest.mark.gpu
def test_reciprocal_on_site_likelihoods_of_a_sweep():
    """pi . x over the node rows a primate sweep produces (phylo_sweep_node): the values pg_rcp is called with in the pass."""
    genome = load_dataset('primate_data')['genome']
    N, S, _ = genome.shape
    K = 64
    rng = np.random.default_rng(6)
    Q = O.get_Q(O.init_y_q())
    p = np.exp(rng.normal(size=4) * 0.5)
    pi = (p / p.sum())[None, :]
    lik = []
    with _ffi.Context(K, N, S) as c:
        c.set_leaves(genome)
        c.set_model(Q, pi, np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        c.sweep(11)
        for r in range(N - 1):
            for k in (0, K // 3, K - 1):
                lik.append(c.sweep_node(r, k) @ pi[0])
        lik = np.concatenate(lik)
        assert np.all(lik > 0) and np.all(np.isfinite(lik))
        worst = int(_ulps(c.math_probe(5, lik), 1.0 / lik).max())
    print('pg_rcp: worst %d ulp on %d site likelihoods in [%.3g, %.3g]' % (worst, lik.size, lik.min(), lik.max()))
    assert worst <= 2                              # worst seen: 0 ulp on 29 634 likelihoods in [4e-13, 1]
