"""The AU test's host side, no GPU: treetests.au_scales, au_fit and au_test -- the weighted least squares
fit of z_k = d / sigma_k + c sigma_k -- on proportions generated exactly from the model, against numpy.linalg.lstsq, on a
simulated half plane and on degenerate rows; and runner.py's parser for --tree_tests_au.

Every test here needs phylo_amd.treetests.au_fit: AttributeError without it."""
import os
import sys
from statistics import NormalDist

import numpy as np
import pytest

from phylo_amd import treetests as TT

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N = NormalDist()
Phi = np.vectorize(N.cdf)


def test_au_scales():
    sc = TT.au_scales(1949, 'default')
    np.testing.assert_allclose(sc['r'], np.arange(5, 15) / 10.0, rtol=0, atol=1e-15)
    assert sc['draws'].dtype == np.int32
    assert sc['draws'].tolist() == [975, 1169, 1364, 1559, 1754, 1949, 2144, 2339, 2534, 2729]      # floor(r S + 0.5)
    np.testing.assert_array_equal(sc['sigma2'], 1949.0 / sc['draws'])                               # from the draws, not from r
    assert sc['sigma2'][5] == 1.0 and sc['sigma2'][0] != 2.0
    sc = TT.au_scales(37, '0.5,1,1.4')
    assert sc['draws'].tolist() == [19, 37, 52] and sc['r'].tolist() == [0.5, 1.0, 1.4]
    assert TT.au_scales(3, '0.01,1')['draws'].tolist() == [1, 3]                                    # at least one draw
    for bad in ('', 'x', '0.5,', '0.5,-1', '0,1', 'nan,1', 'inf,1', '1', '1,1', ','.join(['0.5', '1.0'] * 33)):
        with pytest.raises(ValueError):
            TT.au_scales(100, bad)
    with pytest.raises(ValueError, match='distinct'):
        TT.au_scales(1, 'default')                                                                  # every scale draws one site
    with pytest.raises(ValueError, match='65535'):
        TT.au_scales(60000, 'default')                                                              # 1.4 x 60000 > 65535
    assert TT.au_scales(46810, 'default')['draws'].max() == 65534


@pytest.mark.parametrize("d,c", [(1.3, 0.4), (-0.5, 0.2), (2.5, -0.3)])
def test_fit_recovers_exact_proportions(d, c):
    s2 = TT.au_scales(1949, 'default')['sigma2']
    sg = np.sqrt(s2)
    bp = 1.0 - Phi(d / sg + c * sg)
    for B in (1000, 10000):
        f = TT.au_fit(bp, s2, B)
        assert f['au_ok'] and f['df'] == 8
        assert abs(f['d'] - d) <= 1e-12 and abs(f['c'] - c) <= 1e-12 and abs(f['p_au'] - N.cdf(c - d)) <= 1e-12
        assert f['rss'] <= 1e-12 and f['se_au'] > 0


def lstsq_fit(bp, s2, B):
    """the same fit by numpy.linalg.lstsq on the sqrt(w)-scaled system"""
    use = (bp > 0) & (bp < 1)
    p, sg = bp[use], np.sqrt(s2[use])
    z = np.array([-N.inv_cdf(v) for v in p])
    w = B * np.array([N.pdf(v) for v in z]) ** 2 / (p * (1 - p))
    X = np.stack([1.0 / sg, sg], axis=1)
    sw = np.sqrt(w)
    beta = np.linalg.lstsq(X * sw[:, None], z * sw, rcond=None)[0]
    V = np.linalg.inv(X.T @ (X * w[:, None]))
    res = z - X @ beta
    return {'d': beta[0], 'c': beta[1], 'p_au': N.cdf(beta[1] - beta[0]),
            'se_au': N.pdf(beta[0] - beta[1]) * np.sqrt(V[0, 0] + V[1, 1] - 2 * V[0, 1]), 'rss': float(np.sum(w * res * res))}


def test_fit_is_numpy_lstsq():
    s2 = TT.au_scales(1949, 'default')['sigma2']
    rng = np.random.default_rng(3)
    B = 2000
    for _ in range(20):
        d, c = rng.uniform(-1.0, 2.5), rng.uniform(-0.5, 0.5)
        bp = rng.binomial(B, 1.0 - Phi(d / np.sqrt(s2) + c * np.sqrt(s2))) / B       # noisy proportions, some of them 0 or 1
        if ((bp > 0) & (bp < 1)).sum() < 2:
            continue
        got, want = TT.au_fit(bp, s2, B), lstsq_fit(bp, s2, B)
        assert got['au_ok'] and got['df'] == int(((bp > 0) & (bp < 1)).sum()) - 2
        for key in ('d', 'c', 'p_au', 'se_au', 'rss'):
            assert abs(got[key] - want[key]) <= 1e-10 * max(1.0, abs(want[key])), key


def test_half_plane_simulation():
    """the hypothesis region is a half plane at distance d = 1.5: no curvature, so c is near 0 and p_au near 1 - Phi(1.5)"""
    sc = TT.au_scales(1949, 'default')
    rng = np.random.default_rng(1)
    B, d = 10000, 1.5
    wins = np.array([int(np.count_nonzero(d + np.sqrt(s) * rng.standard_normal(B) < 0)) for s in sc['sigma2']])
    out = TT.au_test(np.stack([wins, B - wins], axis=1), sc['sigma2'], B)
    p, se = out['p_au'][0], out['se_au'][0]
    assert out['au_ok'].all() and abs(out['c'][0]) < 0.1 and abs(out['d'][0] - d) < 0.1
    assert abs(p - (1 - N.cdf(1.5))) <= 4 * se and 0 < se < 0.01
    assert abs(out['p_au'][1] - N.cdf(1.5)) <= 4 * out['se_au'][1]                 # the complement: d = -1.5
    np.testing.assert_array_equal(out['bp'][:, 0], wins / B)


def test_degenerate_rows():
    s2 = TT.au_scales(1949, 'default')['sigma2']
    B = 100
    wins = np.zeros((10, 4), dtype=np.int64)
    wins[:, 1] = B - 7                                   # tree 0 never wins; tree 1 nearly always; tree 2 at one scale only ...
    wins[:, 3] = 7
    wins[2, 2], wins[2, 3] = 3, 4                        # ... (taken from tree 3, so that every scale still adds up to B)
    out = TT.au_test(wins, s2, B)
    assert out['au_ok'].tolist() == [False, True, False, True]
    assert out['p_au'][0] == 0.0 and out['p_au'][2] == 0.0          # the bp at sigma2 = 1 (scale 5), where tree 2 has no win
    assert np.isnan(out['se_au'][[0, 2]]).all() and np.isnan(out['d'][[0, 2]]).all() and np.isnan(out['c'][[0, 2]]).all()
    assert out['df'].tolist() == [-2, 8, -1, 8]
    always = TT.au_fit(np.ones(10), s2, B)
    assert always['p_au'] == 1.0 and not always['au_ok']
    one = TT.au_fit(np.array([0, 0, 0, 0, 0, 0.25, 0, 0, 0, 0]), s2, B)
    assert one['p_au'] == 0.25 and not one['au_ok'] and one['df'] == -1
    two = TT.au_fit(np.array([0, 0, 0, 0, 0, 0.25, 0.5, 1, 1, 1]), s2, B)          # two usable scales: an exact fit, df = 0
    assert two['au_ok'] and two['df'] == 0 and two['rss'] <= 1e-20
    same = TT.au_fit(np.array([0.2, 0.3]), np.array([1.0, 1.0]), B)              # two usable scales of ONE sigma: no fit
    assert not same['au_ok'] and same['p_au'] == 0.2
    for bad in (lambda: TT.au_fit([0.5, 1.5], [1.0, 2.0], B), lambda: TT.au_fit([0.5], [1.0, 2.0], B), lambda: TT.au_fit([0.5, 0.5], [1.0, 0.0], B),
                lambda: TT.au_test(np.full((10, 2), B), s2, B), lambda: TT.au_test(np.zeros((3, 2)), s2, B)):
        with pytest.raises(ValueError):
            bad()


def test_runner_parser(capsys):
    sys.path.insert(0, ROOT)
    try:
        import runner
    finally:
        sys.path.remove(ROOT)
    base = ['--score_trees', 'trees.nwk']
    a = runner.parse_args(base + ['--tree_tests', '100:3', '--tree_tests_au', 'default'])
    assert a.tree_tests_au == 'default' and a.tree_tests == '100:3'
    assert runner.parse_args(base + ['--tree_tests', '100', '--tree_tests_au', '0.5,1,2']).tree_tests_au == '0.5,1,2'
    assert runner.parse_args(base + ['--tree_tests', '100']).tree_tests_au is None
    with pytest.raises(SystemExit):
        runner.parse_args(base + ['--tree_tests_au', 'default'])                     # the flag without --tree_tests
    assert '--tree_tests_au needs --tree_tests' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        runner.parse_args(base + ['--tree_tests', '100', '--tree_tests_au', '0.5,zero'])
    assert '--tree_tests_au:' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        runner.parse_args(base + ['--tree_tests', '100', '--tree_tests_au', '1'])      # one scale fits nothing
    assert '--tree_tests_au:' in capsys.readouterr().err
