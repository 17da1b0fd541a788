"""Ancestral states and site-rate posteriors under rate mixtures without a GPU: the NumPy restatement of
phylo_trees_ancestral_rates' contract (treeanc_rates_ref.py) against an enumeration of every assignment of internal states per
category and against the same formulas at 50 digits (E_REF_POST, E_REF_CAT, E_REF_RATE, from which the device tolerance follows);
the near-floor allowance; its row sums; the preconditions of the device file's cases; the host half of phylo_treeanc_rates.h under
sanitizers; phylo_amd.ancestral's site-rate functions on hand-made arrays; the runner's parser.

Every test here fails without the feature: on the missing symbol, header, module function or flag."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import treeanc_rates_cases as RC
import treeanc_rates_ref as ARR
import treegrad_edges_cases as GC
import trees_edges_cases as EC
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd import ancestral as A
from test_treeanc_cpu import enumerated
from treeanc_cases import gapped
from treeanc_rates_cases import MIX_I_G4, MIXTURES, PRIOR, TOL_ANC_RATES, category_matrices
from trees_cases import random_rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- (a) -----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported():
    assert 'phylo_trees_ancestral_rates' in _ffi.EXPORTS
    assert _ffi.ANC_NOSTATE == A.NOSTATE == ARR.NOSTATE == 255
    with open(os.path.join(ROOT, 'include', 'phylo_hip.h')) as f:
        head = f.read()
    assert '#define PHYLO_ANC_NOSTATE 255' in head and 'int phylo_trees_ancestral_rates(' in head
    assert callable(_ffi.Context.trees_ancestral_rates)


# ---- (b) the restatement computes mixture marginals: every assignment of internal states enumerated, per category -----------------
@pytest.mark.parametrize("N", [3, 4, 5])
@pytest.mark.parametrize("jc", [False, True], ids=['gtr', 'jc'])
@pytest.mark.parametrize("mix", ['C5', 'C3z'])
def test_reference_computes_mixture_marginals(N, jc, mix):
    S = 6
    rng = np.random.default_rng(10 * N + jc)
    g = gapped(N, S, rng)
    g[1] = rng.uniform(0.05, 1.0, size=(S, 4))             # one generic row
    Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
    rates, weights = MIXTURES[mix]
    C = rates.size
    worst = 0.0
    for _ in range(3):
        child, blen = random_rows(N, rng)
        M = category_matrices(Q, blen, rates)
        ref = ARR.tree_ancestral_rates(child, M, PRIOR, g, rates, weights)
        num, L = np.zeros((N - 1, S, 4)), np.zeros((C, S))
        for c in range(C):
            with np.errstate(invalid='ignore'):
                post_c, L[c] = enumerated(child, M[c], PRIOR, g)      # (NaN where L_c = 0: the rate-0 category at a variable site)
                num += weights[c] * np.where(L[c][None, :, None] > 0, post_c * L[c][None, :, None], 0.0)      # num_c = post_c L_c (0 where L_c = 0)
        m = (weights[:, None] * L).sum(axis=0)
        want = {'post': num / m[None, :, None], 'catpost': weights[:, None] * L / m[None, :], 'm': m}
        want['siterate'] = (rates[:, None] * want['catpost']).sum(axis=0)
        for key in ('m', 'post', 'catpost', 'siterate'):
            np.testing.assert_allclose(ref[key], want[key], rtol=1e-13, atol=1e-300, err_msg=key)
            worst = max(worst, float(np.max(np.abs(ref[key] - want[key]) / np.maximum(np.abs(want[key]), 1e-300))))
        np.testing.assert_array_equal(ref['state'], np.argmax(ref['post'], axis=-1))
        np.testing.assert_array_equal(ref['pmax'], ref['post'].max(axis=-1))
        if mix == 'C3z':
            assert (ref['catpost'][1] == 0).all()          # the zero weight: an ordinary category of posterior 0
    print("restatement against the enumeration (%s): worst relative difference %.3g" % (mix, worst))


# ---- (c), (e) the same formulas at 50 digits: E_REF_*; the row sums ------------------------------------------------------------------
def mp_cases():
    N, S = 5, 8
    rates, weights = MIX_I_G4
    for seed in range(20):
        for jc in (False, True):
            rng = np.random.default_rng(seed)
            g = gapped(N, S, rng)
            Q = O.jc_Q() if jc else O.get_Q(rng.normal(size=(4, 4)))
            child, blen = random_rows(N, rng)
            yield child, category_matrices(Q, blen, rates), g


def test_reference_against_mpmath():
    """N = 5, S = 8, gaps; 20 random trees under a GTR-like Q and under JC69 (section 15's recipe) under MIX_I_G4.  The worst
    |reference - 50-digit value| of post, catpost and siterate in units of |value| 2^-53 (every term is non-negative: nothing
    cancels) is the restatement's own error, from which TOL_ANC_RATES = 8 max(E) 2^-53 follows.  Measured here: post 6.90,
    catpost 6.86, siterate 3.65; sites with f_0 = 0 are among them."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    rates, weights = MIX_I_G4
    worst = {'post': 0.0, 'catpost': 0.0, 'siterate': 0.0}
    zero_f0 = 0
    for child, M, g in mp_cases():
        ref = ARR.tree_ancestral_rates(child, M, PRIOR, g, rates, weights)
        zero_f0 += int((ref['f'][0] == 0).sum())
        got = RC.measure(mp, child, M, g, rates, weights, ref)
        assert got['subnormal_f'] == 0
        for k in worst:
            assert got[k] == got[k + '_raw']               # far from the floor the allowance is nothing
            worst[k] = max(worst[k], got[k])
    print("reference against 50 digits: post %.3f, catpost %.3f, siterate %.3f units of |value| 2^-53 (recorded %g, %g, %g; "
          "TOL_ANC_RATES = %.3g); %d tree-sites with f_0 = 0" % (worst['post'], worst['catpost'], worst['siterate'], RC.E_REF_POST,
                                                                 RC.E_REF_CAT, RC.E_REF_RATE, TOL_ANC_RATES, zero_f0))
    assert zero_f0 > 0
    assert RC.E_REF_POST / 2 <= worst['post'] <= RC.E_REF_POST
    assert RC.E_REF_CAT / 2 <= worst['catpost'] <= RC.E_REF_CAT
    assert RC.E_REF_RATE / 2 <= worst['siterate'] <= RC.E_REF_RATE
    assert TOL_ANC_RATES == 8 * max(RC.E_REF_POST, RC.E_REF_CAT, RC.E_REF_RATE) * 2.0 ** -53


def test_reference_posteriors_sum_to_one():
    """neither post nor catpost is renormalised: the restatement's worst |sum_j post_j - 1| and |sum_c catpost_c - 1| over the
    cases of (c) are measured, recorded (SUM_ERR_POST = 6 * 2^-53, SUM_ERR_CAT = 2 * 2^-53) and held at 8 times that"""
    rates, weights = MIX_I_G4
    wp = wc = 0.0
    for child, M, g in mp_cases():
        ref = ARR.tree_ancestral_rates(child, M, PRIOR, g, rates, weights)
        wp = max(wp, float(np.abs(ref['post'].sum(axis=-1) - 1.0).max()))
        wc = max(wc, float(np.abs(ref['catpost'].sum(axis=0) - 1.0).max()))
    print("worst |sum_j post_j - 1| = %.2f * 2^-53 (recorded %.0f), worst |sum_c catpost_c - 1| = %.2f * 2^-53 (recorded %.0f)"
          % (wp * 2.0 ** 53, RC.SUM_ERR_POST * 2.0 ** 53, wc * 2.0 ** 53, RC.SUM_ERR_CAT * 2.0 ** 53))
    assert wp <= RC.SUM_ERR_POST and wc <= RC.SUM_ERR_CAT              # the recorded values are what was measured
    assert RC.SUM_TOL_POST == 8 * RC.SUM_ERR_POST and RC.SUM_TOL_CAT == 8 * RC.SUM_ERR_CAT


@pytest.mark.parametrize("name", list(RC.E_REF_BIG))
def test_reference_against_mpmath_big(name):
    """above 128 taxa (section 13b's recipe: tree 0 at four sites): the restatement's error against 50 digits, net of the absolute
    allowance, stays at or below the recorded E_REF_BIG and above half of it"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    got = RC.measure_big(mp, name)
    print("%s: post %.2f (raw %.3g), catpost %.2f (raw %.3g), siterate %.2f (raw %.3g) units of |value| 2^-53; %d subnormal category factors"
          % (name, got['post'], got['post_raw'], got['catpost'], got['catpost_raw'], got['siterate'], got['siterate_raw'], got['subnormal_f']))
    worst = max(got['post'], got['catpost'], got['siterate'])
    assert RC.E_REF_BIG[name] / 2 <= worst <= RC.E_REF_BIG[name]


# ---- the NaN rule, per site ---------------------------------------------------------------------------------------------------------
def test_reference_nan_rule_is_per_site():
    rng = np.random.default_rng(5)
    N, S = 5, 6
    g = gapped(N, S, rng)
    child, blen = random_rows(N, rng)
    rates, weights = MIX_I_G4
    M = category_matrices(O.get_Q(rng.normal(size=(4, 4))), blen, rates)
    ref = ARR.tree_ancestral_rates(child, M, PRIOR, g, rates, weights)
    g2 = g.copy()
    g2[0, 3] *= 2.0 ** -1021                                # scales that site's value below 2^-1020
    g2[1, 4] = 0.0                                         # and one site has no likelihood at all
    got = ARR.tree_ancestral_rates(child, M, PRIOR, g2, rates, weights)
    assert 0 < got['m'][3] < ARR.FLOOR and got['m'][4] == 0.0
    assert np.isnan(got['post'][:, 3:5]).all() and (got['state'][:, 3:5] == ARR.NOSTATE).all() and np.isnan(got['pmax'][:, 3:5]).all()
    assert np.isnan(got['catpost'][:, 3:5]).all() and np.isnan(got['siterate'][3:5]).all()
    keep = [0, 1, 2, 5]
    np.testing.assert_array_equal(bits(got['post'][:, keep]), bits(ref['post'][:, keep]))
    np.testing.assert_array_equal(got['state'][:, keep], ref['state'][:, keep])
    np.testing.assert_array_equal(bits(got['catpost'][:, keep]), bits(ref['catpost'][:, keep]))
    np.testing.assert_array_equal(bits(got['siterate'][keep]), bits(ref['siterate'][keep]))
    assert (A.category_states(got['catpost'])[3:5] == A.NOSTATE).all()


# ---- (d) the near-floor allowance ---------------------------------------------------------------------------------------------------
def test_near_floor_allowance():
    """section 13's scaled generic alignment under MIX_I_G4 against its unscaled twin, on the restatement alone (under
    treegrad_edges_cases.hardware_fma, as the device file restates it): where the scaled sites' m lies in [2^-1020, 2^-1000) every
    entry of the site's column stays within TOL_ANC_RATES max(|value|, TINY) + k 2^-1075 / m_s, k counted in the code
    (treeanc_rates_cases.k_post, k_cat, k_rate); at 2^-900 the plain tolerance holds alone.  Prints the share of the bound used."""
    g, child, blen, Q = EC.scaled_base()
    rates, weights = MIX_I_G4
    M = np.array([category_matrices(Q, b, rates) for b in blen])
    at = list(EC.SCALED_SITES)
    with GC.hardware_fma():
        ref0 = ARR.trees_ancestral_rates(child, M, PRIOR, g, rates, weights)
        assert np.isfinite(ref0['post']).all() and (ref0['m'] > 2.0 ** -200).all()
        for place in EC.IN_RANGE:
            e = EC.scaled_exponents(place, ref0['m'])
            ref = ARR.trees_ancestral_rates(child, M, PRIOR, EC.scaled_leaves(g, e), rates, weights)
            m = ref['m'][:, at]
            assert (m >= ARR.FLOOR).all()
            if place != '2^-900':
                assert (m < 2.0 ** -1000).all()
            xp, xc, xr = RC.allowance(ref['m'], rates, weights)
            if place == '2^-900':
                xp, xc, xr = 0.0 * xp, 0.0 * xc, 0.0 * xr
            for key, extra in (('post', xp[:, None, :, None]), ('catpost', xc), ('siterate', xr)):
                ok, worst = RC.within(ref[key], ref0[key], extra)
                diff = np.abs(ref[key] - ref0[key])
                plain = float((diff / (TOL_ANC_RATES * np.maximum(np.abs(ref0[key]), RC.TINY))).max())
                print("%s %s: %.3g of the bound with the allowance; %.3g of TOL_ANC_RATES max(|value|, TINY) alone" % (place, key, worst, plain))
                assert ok.all(), (place, key, worst)
            np.testing.assert_array_equal(ref['state'], ref0['state'])
    others = [s for s in range(g.shape[1]) if s not in at]
    np.testing.assert_array_equal(bits(ref['post'][:, :, others]), bits(ref0['post'][:, :, others]))
    assert RC.k_post(rates, weights) == pytest.approx(2 + 5) and RC.k_cat(rates, weights).max() <= 6
    assert RC.k_rate(rates, weights) == pytest.approx(5 * float(np.sum(rates * weights)) + float(np.sum(rates)))


# ---- (f) the device file's cases decide their states and categories --------------------------------------------------------------------
def undecided(ref):
    return 1.0 - float(RC.decided(ref['post']).mean()), 1.0 - float(RC.decided(ref['catpost'], axis=-2).mean())


@pytest.mark.parametrize("name", list(RC.CASES))
def test_device_cases_decide_their_states(name):
    """the precondition of the device test's comparison of states and most probable categories: the restatement's two largest
    posteriors differ by more than 2 TOL_ANC_RATES relative at more than 99 % of the node-sites (sites) of every case (scipy's
    matrices here, the device's own there, where it is asserted again)"""
    g, Q, child, blen, jc, tile, rates, weights = RC.case_inputs(name)
    M = np.array([category_matrices(Q, b, rates) for b in blen])
    ref = ARR.trees_ancestral_rates(child, M, PRIOR, g, rates, weights, exact_mix=False)
    assert np.isfinite(ref['post']).all() and np.isfinite(ref['catpost']).all() and (ref['m'] >= RC.TINY).all(), name
    if g.shape[0] > 2:
        assert (blen == 0).any()                            # trees with zero-length branches
    sp, sc = undecided(ref)
    print("%s: %.4f %% of the node-sites and %.4f %% of the sites undecided" % (name, 100 * sp, 100 * sc))
    assert sp < RC.MAX_EXCLUDED and sc < RC.MAX_EXCLUDED, (name, sp, sc)
    assert np.abs(ref['post'].sum(axis=-1) - 1.0).max() <= RC.SUM_TOL_POST and np.abs(ref['catpost'].sum(axis=1) - 1.0).max() <= RC.SUM_TOL_CAT


@pytest.mark.parametrize("name", list(RC.E_REF_BIG))
def test_big_cases_decide_their_states(name):
    g, child, blen, Q, rates, weights, tile = RC.big_case(name)
    M = np.array([category_matrices(Q, b, rates) for b in blen[:1]])
    ref = ARR.trees_ancestral_rates(child[:1], M, PRIOR, g, rates, weights, exact_mix=False)
    assert np.isfinite(ref['post']).all() and (ref['m'] >= RC.TINY).all(), name
    sp, sc = undecided(ref)
    print("%s: %.4f %% of the node-sites and %.4f %% of the sites undecided" % (name, 100 * sp, 100 * sc))
    assert sp < RC.MAX_EXCLUDED and sc < RC.MAX_EXCLUDED, (name, sp, sc)


# ---- (g) the host half under sanitizers --------------------------------------------------------------------------------------------
def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_treeanc_rates.h with a main of its own (tests/treeanc_rates_asan_main.cpp), address and
    undefined-behaviour sanitizers of the host compiler: slab-, output- and env-bound chunks, C = 1 and 16, the growth to one tree
    over 256 MiB, the refusal above 1 GiB, the grid cap at N = 512, C = 16, the mixture checks."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "treeanc_rates_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "treeanc_rates_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout


# ---- (h) phylo_amd.ancestral's site-rate functions on hand-made arrays -------------------------------------------------------------------
def test_category_states_ties_and_nan():
    nan = np.nan
    catpost = np.array([[0.2, 0.5, 0.1, nan, 0.0, 0.3],
                        [0.6, 0.5, 0.1, 0.5, 0.0, nan],
                        [0.2, 0.0, 0.8, 0.5, 0.0, nan]])     # [C = 3][S = 6]
    cat = A.category_states(catpost)
    np.testing.assert_array_equal(cat, [1, 0, 2, 255, 0, 255])           # ties: the lowest c; any NaN: none
    assert cat.dtype == np.uint8
    np.testing.assert_array_equal(A.category_states(np.stack([catpost, catpost[::-1]])), [[1, 0, 2, 255, 0, 255], [1, 1, 0, 255, 0, 255]])
    np.testing.assert_array_equal(A.category_states(np.array([[1.0, nan]])), [0, 255])          # one category
    with pytest.raises(ValueError):
        A.category_states(np.array([0.5, 0.5]))


def test_summarise_rates_excludes_and_counts_nan_sites():
    nan = np.nan
    siterate = np.array([[0.5, 1.5, 1.0, nan, 2.0], [nan, nan, nan, nan, nan]])
    catpost = np.array([[[0.9, 0.1, 0.5, nan, 0.0], [0.1, 0.9, 0.5, nan, 1.0]], np.full((2, 5), nan)])
    sm = A.summarise_rates(siterate, catpost, quantiles=(0.0, 0.5, 1.0))
    np.testing.assert_array_equal(sm['n_nan'], [1, 5])
    assert sm['mean_rate'][0] == pytest.approx(1.25) and np.isnan(sm['mean_rate'][1])
    np.testing.assert_allclose(sm['quantiles'][0], [0.5, 1.25, 2.0])
    np.testing.assert_allclose(sm['cat_share'][0], [0.5, 0.5])           # sites 0 and 2 (a tie: the lowest) against 1 and 4
    assert np.isnan(sm['quantiles'][1]).all() and np.isnan(sm['cat_share'][1]).all() and sm['q'] == (0.0, 0.5, 1.0)
    assert len(A.summarise_rates(siterate, catpost)['q']) == 5
    with pytest.raises(ValueError):
        A.summarise_rates(siterate[0], catpost)


def test_site_rates_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    T, C, S = 3, 4, 9
    catpost = rng.random((T, C, S)) * 10.0 ** rng.integers(-300, 1, size=(T, C, S))
    siterate = rng.random((T, S)) * 3
    catpost[1, :, 4] = np.nan
    siterate[1, 4] = np.nan
    catpost[2, 0, 0] = 5e-324                              # the smallest subnormal
    siterate[0, 0] = 0.1 + 0.2                             # 0.30000000000000004: repr keeps every bit
    path = str(tmp_path / 'site_rates.tsv')
    A.write_site_rates(path, [7, 2, 5], siterate, catpost)
    back = A.read_site_rates(path)
    np.testing.assert_array_equal(back['trees'], [7, 2, 5])
    np.testing.assert_array_equal(bits(back['siterate']), bits(siterate))
    np.testing.assert_array_equal(bits(back['catpost']), bits(catpost))
    np.testing.assert_array_equal(back['cat'], A.category_states(catpost))
    assert back['cat'][1, 4] == A.NOSTATE and back['cat'].dtype == np.uint8
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == 'tree\tsite\trate\tcat\tp0\tp1\tp2\tp3' and len(lines) == 1 + T * S
    assert lines[1].split('\t')[:3] == ['7', '0', '0.30000000000000004']
    with pytest.raises(ValueError):
        A.write_site_rates(path, [1, 2], siterate, catpost)


# ---- (i) the runner's parser ----------------------------------------------------------------------------------------------------------
def runner_module():
    sys.path.insert(0, ROOT)
    try:
        import runner
    finally:
        sys.path.remove(ROOT)
    return runner


RATES = ['--score_rates', 'gamma:0.5:4']


@pytest.mark.parametrize("argv,what", [
    (['--score_ancestral_rates', '2'] + RATES, '--score_rates needs --score_trees'),
    (['--score_ancestral_rates', '2'], '--score_ancestral_rates needs --score_trees'),
    (['--score_ancestral_rates', '2', '--score_trees', 'x.nwk'], '--score_ancestral_rates needs --score_rates'),
    (['--score_ancestral_rates', '2', '--score_trees', 'x.nwk', '--score_ancestral', '2'] + RATES, 'exclude one another'),
    (['--score_ancestral_rates', '2', '--score_trees', 'x.nwk', '--score_ancestral', '2'], 'exclude one another'),
    (['--score_ancestral_rates', '0', '--score_trees', 'x.nwk'] + RATES, 'K >= 1'),
    (['--score_ancestral', '2', '--score_trees', 'x.nwk'] + RATES, 'not built for rate mixtures'),
    (['--score_ancestral', '2', '--score_trees', 'x.nwk'] + RATES, 'use --score_ancestral_rates'),
])
def test_runner_parser_errors(argv, what, capsys):
    runner = runner_module()
    with pytest.raises(SystemExit) as e:
        runner.parse_args(['--dataset', 'primate_data_wang'] + argv)
    assert e.value.code == 2 and what in capsys.readouterr().err


def test_runner_parser_accepts():
    runner = runner_module()
    base = ['--dataset', 'primate_data_wang', '--score_trees', 'x.nwk', '--score_ancestral_rates', '3'] + RATES
    assert runner.parse_args(base).score_ancestral_rates == 3
    assert runner.parse_args(base + ['--score_fit', 'branches+alpha']).score_ancestral_rates == 3
    a = runner.parse_args(base + ['--score_fit', 'branches+alpha', '--score_fit_search', 'nni:5'])
    assert a.score_ancestral_rates == 3 and a.score_fit_search == ('nni', 5)
    assert runner.parse_args(base + ['--tree_tests', '100']).score_ancestral_rates == 3
    assert runner.parse_args(['--dataset', 'primate_data_wang']).score_ancestral_rates is None
    assert '--score_ancestral_rates' in runner.__doc__
