"""phylo_amd.rates without a GPU: the discrete Gamma rates against scipy's incomplete gamma functions and
Yang's published values, rate_model, site_rates, the runner's --score_rates parsing, and the ABI's new export.

Every test here needs phylo_amd.rates or --score_rates: ImportError, AttributeError or a parser error without them."""
import os
import sys

import numpy as np
import pytest
import scipy.special as sp

import rates_ref
from phylo_amd import _ffi
from phylo_amd import rates as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import runner                                              # noqa: E402

ALPHAS = (0.1, 0.5, 1, 5, 100)
CATS = (1, 2, 4, 8)


def scipy_rates(alpha, C, kind):
    if kind == 'median':
        r = sp.gammaincinv(alpha, (2 * np.arange(C) + 1) / (2.0 * C)) / alpha
        return r * C / r.sum()
    q = sp.gammaincinv(alpha, np.arange(1, C) / C)
    cut = np.concatenate([[0.0], sp.gammainc(alpha + 1, q), [1.0]])
    return C * np.diff(cut)


@pytest.mark.parametrize("kind", ['mean', 'median'])
@pytest.mark.parametrize("C", CATS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_discrete_gamma_against_scipy(alpha, C, kind):
    got = R.discrete_gamma(alpha, C, kind=kind)
    ref = scipy_rates(alpha, C, kind)
    print(alpha, C, kind, "max |got - ref| / (1e-9 |ref| + 1e-12) =", np.max(np.abs(got - ref) / (1e-9 * np.abs(ref) + 1e-12)))
    assert got.shape == (C,) and got.dtype == np.float64
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12)
    assert abs(got.mean() - 1.0) <= 1e-12
    assert (np.diff(got) > 0).all() and (got > 0).all()


def test_yangs_values():
    np.testing.assert_array_equal(np.round(R.discrete_gamma(0.5, 4), 8), [0.03338775, 0.25191592, 0.82026848, 2.89442785])


def test_one_category_is_exactly_one():
    for alpha in ALPHAS:
        for kind in ('mean', 'median'):
            r = R.discrete_gamma(alpha, 1, kind=kind)
            assert r.shape == (1,) and r[0] == 1.0


def test_incomplete_gamma_and_its_inverse():
    for a in (0.05, 0.1, 0.5, 1.0, 2.5, 30.0, 101.0):
        for x in (1e-12, 1e-3, 0.3, 1.0, a, a + 1.0, 3 * a + 5, 40.0 + 3 * a):
            assert R.gamma_p(a, x) == pytest.approx(float(sp.gammainc(a, x)), rel=1e-12, abs=1e-300), (a, x)
        for p in (1e-6, 0.125, 0.5, 0.875, 0.999):
            assert R.gamma_p_inv(a, p) == pytest.approx(float(sp.gammaincinv(a, p)), rel=1e-11), (a, p)
    assert R.gamma_p(2.0, 0.0) == 0.0 and R.gamma_p_inv(2.0, 0.0) == 0.0
    for bad in ((0.0, 1.0), (-1.0, 1.0), (1.0, -1.0)):
        with pytest.raises(ValueError):
            R.gamma_p(*bad)
    for bad in ((1.0, 1.0), (1.0, -0.1), (0.0, 0.5)):
        with pytest.raises(ValueError):
            R.gamma_p_inv(*bad)
    for bad in ((0.0, 4), (-1.0, 4), (np.inf, 4), (1.0, 0)):
        with pytest.raises(ValueError):
            R.discrete_gamma(*bad)
    with pytest.raises(ValueError):
        R.discrete_gamma(1.0, 4, kind='mode')


def test_rate_model():
    for alpha in (None,) + ALPHAS:
        for C in CATS:
            for pinv in (0.0, 0.1, 0.35):
                r, w = R.rate_model(alpha, C, pinv)
                n = (1 if alpha is None else C) + (pinv > 0)
                assert r.shape == w.shape == (n,)
                assert abs(w.sum() - 1.0) <= 1e-15 * n
                assert (r == 0).sum() == (1 if pinv > 0 else 0)
                if pinv > 0:
                    assert r[0] == 0.0 and w[0] == pinv
                var = r[r > 0]
                np.testing.assert_array_equal(var, [1.0] if alpha is None else R.discrete_gamma(alpha, C))     # not rescaled
                assert (w[r > 0] == (1.0 - pinv) / var.size).all()
                assert (np.diff(r) > 0).all()
    assert 'NOT rescaled' in ' '.join(R.rate_model.__doc__.split())          # the docstring states the convention
    for bad in (-0.1, 1.0, np.nan):
        with pytest.raises(ValueError):
            R.rate_model(0.5, 4, bad)
    with pytest.raises(ValueError):
        R.rate_model(0.5, 16, 0.1)                           # 17 categories
    assert R.rate_model(0.5, 16)[0].size == R.MAX_CATS == 16


def test_site_rates_against_numpy():
    rng = np.random.default_rng(3)
    r, w = R.rate_model(0.7, 4, 0.2)
    f = rng.random((3, 5, 11)) * np.exp(rng.normal(0, 20, (3, 1, 11)))
    f[1, :, 4] = 0.0
    mean, post = R.site_rates(f, r, w)
    assert mean.shape == (3, 11) and post.shape == (3, 5, 11)
    for t in range(3):
        for s in range(11):
            j = [w[c] * f[t, c, s] for c in range(5)]
            if sum(j) == 0:
                assert np.isnan(mean[t, s]) and np.isnan(post[t, :, s]).all()
                continue
            p = np.array(j) / sum(j)
            np.testing.assert_allclose(post[t, :, s], p, rtol=1e-14)
            assert mean[t, s] == pytest.approx(float((p * r).sum()), rel=1e-13)
    ok = ~np.isnan(mean)
    np.testing.assert_allclose(post.sum(axis=1)[ok], 1.0, rtol=1e-14)
    m1, p1 = R.site_rates(f[0], r, w)                        # one tree: [C][S]
    np.testing.assert_array_equal(m1, mean[0])
    with pytest.raises(ValueError):
        R.site_rates(f[:, :4], r, w)


def test_parse_spec():
    m = R.parse_spec('gamma:0.5:4:0.1')
    r, w = R.rate_model(0.5, 4, 0.1)
    assert m['spec'] == 'gamma:0.5:4:0.1'
    np.testing.assert_array_equal(m['rates'], r)
    np.testing.assert_array_equal(m['weights'], w)
    assert R.parse_spec('gamma:2:3')['rates'].shape == (3,)
    for bad in ('gamma', 'gamma:0.5', 'gamma:x:4', 'gamma:0.5:4.5', 'invgamma:0.5:4', 'gamma:0.5:4:0.1:7', 'gamma:-1:4', 'gamma:0.5:0',
                'gamma:0.5:4:1.0', 'gamma:0.5:17', ''):
        with pytest.raises(ValueError):
            R.parse_spec(bad)


def test_runner_arguments(capsys):
    a = runner.parse_args(['--score_trees', 'trees.nwk', '--score_rates', 'gamma:0.5:4:0.1'])
    assert a.score_rates == 'gamma:0.5:4:0.1' and a.score_trees == 'trees.nwk'
    assert runner.parse_args([]).score_rates is None
    assert runner.parse_args(['--score_trees', 'trees.nwk']).score_rates is None
    for argv, what in ((['--score_rates', 'gamma:0.5:4'], '--score_trees'),
                       (['--score_trees', 'trees.nwk', '--score_rates', 'gamma:0.5'], 'gamma:ALPHA:C'),
                       (['--score_trees', 'trees.nwk', '--score_rates', 'gamma:0:4'], 'alpha'),
                       (['--score_trees', 'trees.nwk', '--score_rates', 'gamma:0.5:4:1.5'], 'pinv')):
        with pytest.raises(SystemExit) as e:
            runner.parse_args(argv)
        assert e.value.code == 2
        assert what in capsys.readouterr().err


def test_mixing_chain_restated():
    """rates_ref.mix is the contract the GPU tests replay: one rounding per step, ascending order"""
    assert rates_ref.fma(2.0 ** 53, 1.0, 1.0) == 2.0 ** 53 and rates_ref.fma(2.0 ** 53 + 2, 1.0, 1.0) == 2.0 ** 53 + 4
    assert rates_ref.fma(1 + 2.0 ** -30, 1 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60        # the product is not rounded first
    w, f = np.array([0.25, 0.5, 0.25]), np.array([[1.0, 3.0], [2.0, 5.0], [4.0, 7.0]])
    np.testing.assert_array_equal(rates_ref.mix(w, f), [2.25, 5.0])
    np.testing.assert_array_equal(rates_ref.mix([1.0], f[:1]), f[0])


def test_the_abi_exports_the_rates_call():
    assert 'phylo_trees_loglik_rates' in _ffi.EXPORTS
    assert hasattr(_ffi.load(), 'phylo_trees_loglik_rates')
    assert hasattr(_ffi.Context, 'trees_loglik_rates')
    with open(os.path.join(ROOT, 'include', 'phylo_hip.h')) as f:
        assert 'int phylo_trees_loglik_rates(' in f.read()
