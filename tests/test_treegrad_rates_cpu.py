"""Gradients under rate mixtures without a GPU: the NumPy restatement of phylo_trees_grad_rates' contract
(treegrad_rates_ref.py) against central differences of its own log-likelihood and against the same formulas at 50 digits;
phylo_amd.rates.rate_model_jacobian and chain; the host half of phylo_treegrad_rates.h under sanitizers.

Every test here fails without phylo_trees_grad_rates in the binding or without phylo_amd.rates.rate_model_jacobian."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import treegrad_rates_ref as TRR
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd import rates as R
from treegrad_rates_cases import E_REF_RATES, MIX_I_G4, category_matrices
from trees_cases import random_rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRIOR = np.array([0.1, 0.2, 0.3, 0.4])


def gtr_Q(seed=7):
    return O.get_Q(np.random.default_rng(seed).normal(size=(4, 4)))


def gapped(N, S, rng):
    codes = rng.integers(0, 5, size=(N, S))
    return np.stack([(codes == b) | (codes == 4) for b in range(4)], axis=-1).astype(np.float64)


def test_symbol_is_exported():
    assert 'phylo_trees_grad_rates' in _ffi.EXPORTS


# ---- (a) central differences of the restatement's own log-likelihood -----------------------------------------------------------
def test_reference_against_central_differences():
    """N = 6, S = 40, gaps, +I+G4, lengths 0.05 + Exp(0.1); the function differenced is the restatement's own loglik (scipy's
    expm on the moved point).  grad, drate and dweight against (f(x + h) - f(x - h)) / 2h with h = 1e-5, curv against the second
    difference with h = 1e-3; asserted at 1e-7 and 1e-3 of (1 + |value|), section 13's figures: a wrong sign, a missing factor
    r_c or w_c, or a swapped category is off by its whole size.  The rate-0 category's drate is one-sided in nature (a rate
    cannot go below 0) but the formula extends: it is differenced with the rate moved to +h and -h all the same, expm taking
    a negative length."""
    N, S = 6, 40
    rng = np.random.default_rng(3)
    g = gapped(N, S, rng)
    Q = gtr_Q()
    child, blen = random_rows(N, rng, zeros=False)
    blen = blen + 0.05
    rates, weights = MIX_I_G4

    def f(b, r, w):
        return TRR.tree_grad_rates(child, category_matrices(Q, b, r), Q, PRIOR, g, b, r, w)

    ref = f(blen, rates, weights)
    ll = ref['loglik']
    worst = {'grad': 0.0, 'curv': 0.0, 'drate': 0.0, 'dweight': 0.0}

    def off(name, fd, val):
        worst[name] = max(worst[name], abs(fd - val) / (1 + abs(fd)))

    for i in range(N - 1):
        for sd in range(2):
            def at(h):
                b = blen.copy()
                b[i, sd] += h
                return f(b, rates, weights)['loglik']
            off('grad', (at(1e-5) - at(-1e-5)) / 2e-5, ref['grad'][i, sd])
            off('curv', (at(1e-3) - 2 * ll + at(-1e-3)) / 1e-6, ref['curv'][i, sd])
    for c in range(rates.size):
        def at_r(h):
            r = rates.copy()
            r[c] += h
            return f(blen, r, weights)['loglik']

        def at_w(h):
            w = weights.copy()
            w[c] += h
            return f(blen, rates, w)['loglik']
        off('drate', (at_r(1e-5) - at_r(-1e-5)) / 2e-5, ref['drate'][c])
        off('dweight', (at_w(1e-5) - at_w(-1e-5)) / 2e-5, ref['dweight'][c])
    print("central differences, off by (of 1 + |value|):", worst)
    assert worst['grad'] <= 1e-7 and worst['drate'] <= 1e-7 and worst['dweight'] <= 1e-7 and worst['curv'] <= 1e-3


# ---- (b) the same formulas at 50 digits: E_REF_RATES ---------------------------------------------------------------------------
def test_reference_against_mpmath():
    """Section 13's recipe under p_inv = 0.1 + Gamma4(alpha = 0.5): N = 5, S = 8, gaps; 20 random trees (zero-length branches
    among them) under a GTR-like Q and under JC69.  The worst |reference - 50-digit value| over every entry of grad, curv, drate
    and dweight, in units of (scale + |value|) 2^-53, is E_REF_RATES (treegrad_rates_cases.py).  Sites at which the invariant
    class has f_0 = 0 are among them (asserted)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    mpf = mp.mpf
    N, S = 5, 8
    rates, weights = MIX_I_G4
    C = rates.size
    worst = {'grad': 0.0, 'curv': 0.0, 'drate': 0.0, 'dweight': 0.0}
    zeros_seen = 0
    for seed in range(20):
        for jc in (False, True):
            rng = np.random.default_rng(seed)
            g = gapped(N, S, rng)
            Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
            child, blen = random_rows(N, rng)
            M = category_matrices(Q, blen, rates)
            ref = TRR.tree_grad_rates(child, M, Q, PRIOR, g, blen, rates, weights)
            zeros_seen += int((ref['f'][0] == 0).sum())
            assert np.isfinite(ref['grad']).all() and np.isfinite(ref['drate']).all()
            Mm = [[[[[mpf(float(v)) for v in r] for r in M[c, i, sd]] for sd in range(2)] for i in range(N - 1)] for c in range(C)]
            Qm = [[mpf(float(v)) for v in r] for r in Q]
            pm = [mpf(float(v)) for v in PRIOR]
            bm = [[mpf(float(v)) for v in row] for row in blen]
            rm, wm = [mpf(float(v)) for v in rates], [mpf(float(v)) for v in weights]
            G = [[mpf(0), mpf(0)] for _ in range(N - 1)]
            Cv = [[mpf(0), mpf(0)] for _ in range(N - 1)]
            Dr, Dw = [mpf(0)] * C, [mpf(0)] * C
            for s in range(S):
                rows = [[mpf(float(v)) for v in g[i, s]] for i in range(N)]
                m, a1, a2, dr, f = TRR.site_terms_rates(child.tolist(), Mm, Qm, pm, rows, bm, rm, wm, mpf(0))
                for i in range(N - 1):
                    for sd in range(2):
                        G[i][sd] += a1[i][sd] / m
                        Cv[i][sd] += a2[i][sd] / m - (a1[i][sd] / m) ** 2
                for c in range(C):
                    Dr[c] += dr[c] / m
                    Dw[c] += f[c] / m

            def err(name, val, exact, scale):
                unit = (mpf(float(scale)) + abs(exact)) * mpf(2) ** -53
                if unit > 0:
                    worst[name] = max(worst[name], float(abs(mpf(float(val)) - exact) / unit))
                else:
                    assert val == 0

            for i in range(N - 1):
                for sd in range(2):
                    err('grad', ref['grad'][i, sd], G[i][sd], ref['scale'][i, sd])
                    err('curv', ref['curv'][i, sd], Cv[i][sd], ref['scale'][i, sd])
            for c in range(C):
                err('drate', ref['drate'][c], Dr[c], ref['drate_scale'][c])
                err('dweight', ref['dweight'][c], Dw[c], ref['dweight'][c])
    top = max(worst.values())
    print("reference against 50 digits, units of (scale + |value|) 2^-53:", worst, "(E_REF_RATES = %g)" % E_REF_RATES)
    assert zeros_seen > 0
    assert E_REF_RATES / 2 <= top <= E_REF_RATES


# ---- (c) the Jacobian of the rate model and the chain rule ---------------------------------------------------------------------
@pytest.mark.parametrize("alpha,C,pinv", [(0.5, 4, 0.1), (2.0, 8, 0.0), (0.1, 4, 0.3), (30.0, 3, 0.0)])
def test_rate_model_jacobian_against_differences(alpha, C, pinv):
    """d rates / d alpha is a central difference of discrete_gamma in log alpha of step rates.JAC_STEP; it is held to the same
    difference at half that step (the two agree to the truncation term, of the order of the step squared) and to a step four
    times as large, loosely; d weights / d p_inv is exact."""
    rates, weights = R.rate_model(alpha, C, pinv, keep_invariant=True)
    dr, dw = R.rate_model_jacobian(alpha, C, pinv, keep_invariant=True)
    assert dr.shape == rates.shape and dw.shape == weights.shape and rates.size == C + 1
    assert dr[0] == 0.0 and dw[0] == 1.0 and (dw[1:] == -1.0 / C).all()
    for h, tol in ((R.JAC_STEP / 2, 1e-6), (4 * R.JAC_STEP, 1e-4)):
        up, dn = R.discrete_gamma(alpha * np.exp(h), C), R.discrete_gamma(alpha * np.exp(-h), C)
        fd = (up - dn) / (2 * h) / alpha
        np.testing.assert_allclose(dr[1:], fd, rtol=0, atol=tol * (1 + np.abs(fd).max()))
    assert abs(dr[1:].sum()) <= 1e-6 * (1 + np.abs(dr).max())             # the mean rate stays 1
    plain_r, plain_w = R.rate_model(alpha, C, pinv)
    if pinv > 0:
        np.testing.assert_array_equal(plain_r, rates)
        np.testing.assert_array_equal(plain_w, weights)
    else:
        np.testing.assert_array_equal(plain_r, rates[1:])
        assert weights[0] == 0.0


def test_chain():
    rng = np.random.default_rng(1)
    drate, dweight = rng.normal(size=(3, 5)), rng.normal(size=(3, 5))
    jac = R.rate_model_jacobian(0.5, 4, 0.1)
    da, dp = R.chain(drate, dweight, jac)
    np.testing.assert_allclose(da, drate @ jac[0], rtol=1e-15)
    np.testing.assert_allclose(dp, dweight @ jac[1], rtol=1e-15)
    jacs = (np.stack([jac[0]] * 3), np.stack([jac[1]] * 3))                # one Jacobian per tree
    da2, dp2 = R.chain(drate, dweight, jacs)
    np.testing.assert_allclose(da2, da, rtol=1e-15)
    np.testing.assert_allclose(dp2, dp, rtol=1e-15)


def test_chain_is_the_derivative_of_the_restatement():
    """d loglik / d alpha and / d p_inv of the restatement through rate_model, against central differences in alpha and p_inv"""
    N, S = 5, 30
    rng = np.random.default_rng(5)
    g = gapped(N, S, rng)
    Q = gtr_Q()
    child, blen = random_rows(N, rng, zeros=False)
    blen = blen + 0.05
    alpha, C, pinv = 0.7, 4, 0.15

    def f(a, p):
        r, w = R.rate_model(a, C, p, keep_invariant=True)
        return TRR.tree_grad_rates(child, category_matrices(Q, blen, r), Q, PRIOR, g, blen, r, w)

    ref = f(alpha, pinv)
    da, dp = R.chain(ref['drate'], ref['dweight'], R.rate_model_jacobian(alpha, C, pinv))
    fa = (f(alpha + 1e-5, pinv)['loglik'] - f(alpha - 1e-5, pinv)['loglik']) / 2e-5
    fp = (f(alpha, pinv + 1e-5)['loglik'] - f(alpha, pinv - 1e-5)['loglik']) / 2e-5
    print("d/d alpha %.10g against %.10g; d/d p_inv %.10g against %.10g" % (da, fa, dp, fp))
    assert abs(da - fa) <= 1e-6 * (1 + abs(fa)) and abs(dp - fp) <= 1e-6 * (1 + abs(fp))


# ---- the host half under sanitizers -------------------------------------------------------------------------------------------
def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_treegrad_rates.h (ptgr_make_plan, ptgr_check_mixture, ptgr_coefficients, ptgr_lds_bytes) with a
    main of its own (tests/treegrad_rates_asan_main.cpp), address and undefined-behaviour sanitizers of the host compiler: host
    code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "treegrad_rates_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "treegrad_rates_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 checks failed" in p.stdout


# ---- (d) the optimiser over lengths and shape -------------------------------------------------------------------------------
def test_optimize_rates_against_lbfgsb():
    """An alignment of 600 sites simulated under Gamma4(alpha = 0.5) along an 8-taxon tree; that tree and its nearest-neighbour
    interchanges, every length off by a factor in [1/2, 2], alpha from 1.0.  Every tree climbs its lengths and its alpha on the
    restatement.  The yardstick is scipy's L-BFGS-B on the same function (the restatement's loglik and its gradient in the
    lengths and log alpha) from three starts per tree -- the perturbed lengths at alpha 1, 0.1 everywhere at alpha 0.3, the
    perturbed lengths at alpha 3 --, by test_treegrad_cpu.py's criterion: 2^-46 relative (1.4e-14) in the log-likelihood.
    Measured here: L-BFGS-B against itself over its starts 2.8e-16 relative at the worst, optimize_rates against its best
    2.8e-16."""
    from scipy.optimize import minimize
    from phylo_amd.treeopt import optimize_rates
    from treegrad_rates_cases import eigen_matrices, fit_case
    N, S, C = 8, 600, 4
    Q = gtr_Q()
    g, child, blen = fit_case(N, S, 99, 8, Q, PRIOR)
    T = child.shape[0]
    assert T >= 5
    calls = [0]

    def mats(b, r):                                                       # (through Q's eigenvectors: many thousands of matrices)
        return eigen_matrices(Q, np.asarray(r)[:, None, None] * b)

    def fn(b, rates, weights):
        calls[0] += 1
        res = [TRR.tree_grad_rates(child[t], mats(b[t], rates[t]), Q, PRIOR, g, b[t], rates[t], weights[t], exact_mix=False) for t in range(T)]
        return tuple(np.array([r[k] for r in res]) for k in ('loglik', 'grad', 'curv', 'drate', 'dweight'))

    out = optimize_rates(fn, child, blen, 1.0, C)
    print("iterations", out['iterations'], "alpha", out['alpha'], "calls", calls[0])
    assert calls[0] == out['history'].shape[0]                            # one call per iteration, and the start
    assert (np.diff(out['history'], axis=0) >= 0).all()                  # every tree's sequence is non-decreasing
    assert out['converged'].all()
    assert (out['alpha'] > 0.02).all() and (out['alpha'] < 100).all() and out['pinv'] is None
    assert out['rates'].shape == (T, C) and out['blen'].shape == blen.shape and out['grad_model'].shape == (T, 1)
    free = ~((out['blen'] <= 1e-8) & (out['grad'] < 0))
    assert (np.abs(out['grad'][free]) <= 1e-6).all() and (np.abs(out['grad_model']) <= 1e-6).all()
    for t in range(T):
        np.testing.assert_array_equal(out['rates'][t], R.rate_model(out['alpha'][t], C)[0])
    worst_self = worst = 0.0
    for t in range(T):
        def f(x):
            b, a = x[:-1].reshape(N - 1, 2), float(np.exp(x[-1]))
            r, w = R.rate_model(a, C)
            res = TRR.tree_grad_rates(child[t], mats(b, r), Q, PRIOR, g, b, r, w, exact_mix=False)
            da, _ = R.chain(res['drate'], res['dweight'], R.rate_model_jacobian(a, C))
            return -res['loglik'], -np.concatenate([res['grad'].ravel(), [da * a]])
        starts = [np.concatenate([blen[t].ravel(), [0.0]]), np.concatenate([np.full(2 * N - 2, 0.1), [np.log(0.3)]]),
                  np.concatenate([blen[t].ravel(), [np.log(3.0)]])]
        bounds = [(1e-8, 100.0)] * (2 * N - 2) + [(np.log(0.02), np.log(100.0))]
        runs = [minimize(f, x0, jac=True, method='L-BFGS-B', bounds=bounds, options=dict(gtol=1e-6, ftol=0, maxiter=1000)) for x0 in starts]
        funs = [r.fun for r in runs]
        worst_self = max(worst_self, (max(funs) - min(funs)) / abs(min(funs)))
        best = -min(funs)
        worst = max(worst, abs(out['loglik'][t] - best) / abs(best))
    print("L-BFGS-B against itself over three starts: %.3g relative; optimize_rates against its best: %.3g" % (worst_self, worst))
    assert worst_self <= 2.0 ** -46 and worst <= 2.0 ** -46


def test_optimize_rates_fits_pinv_and_keeps_bounds():
    """a concave toy function of two lengths, log alpha and p_inv whose optimum lies outside the bounds of both model
    coordinates: they end at their bounds, the tree converges, and fit=() leaves the model where it was"""
    from phylo_amd.treeopt import optimize_rates
    target = np.array([0.3, 0.7])

    def make(alpha_t, pinv_t):
        def fn(b, rates, weights):
            # a "likelihood" that reads alpha and p_inv back from the mixture: weights[0] = p_inv, rates from discrete_gamma
            p = weights[:, 0]
            a = np.array([alphas[tuple(r)] for r in rates])
            ll = -((b.reshape(-1, 2) - target) ** 2).sum(axis=1) - (np.log(a) - np.log(alpha_t)) ** 2 - (p - pinv_t) ** 2
            g = -2 * (b - target.reshape(1, 1, 2))
            # d/d rate and d/d weight such that chain gives d/d alpha and d/d p_inv: put everything on category 0's weight and
            # spread d/d alpha over the rates by least squares against the Jacobian
            drate, dweight = np.zeros_like(rates), np.zeros_like(weights)
            for t in range(len(a)):
                dr, dw = R.rate_model_jacobian(a[t], 4, p[t], keep_invariant=True)
                drate[t] = dr * (-2 * (np.log(a[t]) - np.log(alpha_t)) / a[t]) / (dr @ dr)
                dweight[t] = dw * (-2 * (p[t] - pinv_t)) / (dw @ dw)
            return ll, g, np.full(b.shape, -2.0), drate, dweight
        return fn

    alphas = {}
    real = R.rate_model

    def remember(alpha=None, C=4, pinv=0.0, keep_invariant=False):
        r, w = real(alpha, C, pinv, keep_invariant)
        alphas[tuple(r)] = alpha
        return r, w

    R.rate_model = remember
    try:
        out = optimize_rates(make(1e-3, -0.5), None, np.full((1, 1, 2), 0.5), 1.0, 4, pinv0=0.2, fit=('alpha', 'pinv'))
        assert out['converged'].all() and (np.diff(out['history'], axis=0) >= 0).all()
        np.testing.assert_allclose(out['blen'], [[[0.3, 0.7]]], rtol=1e-6)
        np.testing.assert_allclose(out['alpha'], [0.02], rtol=1e-12)
        assert out['pinv'][0] == 0.0 and out['weights'][0, 0] == 0.0 and out['rates'].shape == (1, 5)
        out = optimize_rates(make(1e3, 2.0), None, np.full((1, 1, 2), 0.5), 1.0, 4, pinv0=0.2, fit=('alpha', 'pinv'))
        assert out['converged'].all()
        np.testing.assert_allclose(out['alpha'], [100.0], rtol=1e-12)
        np.testing.assert_allclose(out['pinv'], [0.99], rtol=1e-12)
        out = optimize_rates(make(1e3, 2.0), None, np.full((1, 1, 2), 0.5), 1.0, 4, pinv0=0.2, fit=())
        assert out['converged'].all() and out['alpha'][0] == 1.0 and out['pinv'][0] == 0.2 and out['grad_model'].shape == (1, 0)
    finally:
        R.rate_model = real
    with pytest.raises(ValueError):
        optimize_rates(make(1.0, 0.1), None, np.full((1, 1, 2), 0.5), 1.0, 4, fit=('beta',))


# ---- (e) the large case of the device tests stays in range ---------------------------------------------------------------------
def test_large_case_site_values_stay_in_range():
    """N = 512 under 16 categories (test_gpu_treegrad_rates.py): every site value of every tree stays above 2^-1000, by ordinary
    matrix products on the CPU, so that the NaN rule stays out of that comparison"""
    import trees_edges_cases as EC
    from treegrad_rates_cases import large_case, plain_site_values
    g, child, blen, Q, rates, weights = large_case()
    assert child.shape == (11, 511, 2) and g.shape == (512, 65, 4) and rates.size == 16 and rates[0] == 0.0
    worst = min(plain_site_values(child[t], blen[t], Q, EC.PRIOR, g, rates, weights).min() for t in range(child.shape[0]))
    print("smallest site value: 2^%.1f" % np.log2(worst))
    assert worst > EC.ROOMY


# ---- (f) the runner's parser ---------------------------------------------------------------------------------------------------
def _runner():
    import sys
    sys.path.insert(0, ROOT)
    try:
        import runner
    finally:
        sys.path.remove(ROOT)
    return runner


@pytest.mark.parametrize("argv,what", [
    (['--score_fit', 'branches'], '--score_fit needs --score_trees'),
    (['--score_fit', 'branches', '--score_trees', 'x.nwk'], '--score_fit needs --score_trees FILE and --score_rates'),
    (['--score_fit', 'branches', '--score_rates', 'gamma:0.5:4'], '--score_rates needs --score_trees'),
    (['--score_fit', 'branches+alpha', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4', '--score_opt', 'true'], 'not built for rate mixtures'),
    (['--score_fit', 'lengths', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4'], 'invalid choice'),
    (['--score_fit', 'branches+alpha', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:1'], 'no shape to fit'),
    (['--score_opt', 'true', '--score_trees', 'x.nwk', '--score_rates', 'gamma:0.5:4'], '--score_fit branches'),
])
def test_runner_parser_errors(argv, what, capsys):
    runner = _runner()
    with pytest.raises(SystemExit) as e:
        runner.parse_args(['--dataset', 'primate_data_wang'] + argv)
    assert e.value.code == 2 and what in capsys.readouterr().err


def test_runner_parser_accepts_score_fit():
    runner = _runner()
    base = ['--dataset', 'primate_data_wang', '--score_trees', 'x.nwk']
    for mode in ('branches', 'branches+alpha', 'branches+alpha+pinv'):
        for spec in ('gamma:0.5:4', 'gamma:0.5:4:0.1'):
            a = runner.parse_args(base + ['--score_rates', spec, '--score_fit', mode, '--tree_tests', '100:1'])
            assert a.score_fit == mode and a.score_opt is False
    assert runner.parse_args(base + ['--score_rates', 'gamma:0.5:1', '--score_fit', 'branches']).score_fit == 'branches'
    assert runner.parse_args(base).score_fit is None and runner.parse_args(['--dataset', 'primate_data_wang']).score_fit is None
