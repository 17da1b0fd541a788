"""The edges of phylo_trees_grad_rates and phylo_trees_grad_model without a GPU (DESIGN.md sections 13b, 13c; inputs:
treegrad_edges_cases.py, trees_edges_cases.py): the restatements against the same formulas at 50 digits on trees of 129 to 512
taxa (E_REF_RATES_BIG, E_REF_MODEL_BIG), every precondition that the two device files assert again before they compare
anything -- site values clear of the floor under the mixtures, the places of the scaled sites, normal category factors at 2^-900
and subnormal ones at the floor --, and section 13b's near-floor bound of drate and dweight held from both sides: the
restatement on the scaled alignment stays inside it against the unscaled one, and does NOT stay inside plain TOL_RATES."""
import functools

import numpy as np
import pytest

import treegrad_edges_cases as GC
import treegrad_model_ref as MR
import treegrad_rates_ref as TRR
import treegrad_ref as TR
import trees_edges_cases as EC
from test_gpu_trees_loglik import bits
from treegrad_cases import branch_matrices
from treegrad_model_ref import E_REF_MODEL, TOL_MODEL
from treegrad_rates_cases import E_REF_RATES, MIX_I_G4, TOL_RATES, category_matrices, plain_site_values
from trees_edges_cases import FLOOR, PRIOR, ROOMY

AT = list(EC.SCALED_SITES)
UNIT = 2.0 ** -53


# ---- A. the strip cases are what their names say -----------------------------------------------------------------------------------
def test_strip_cases():
    """one item under the default tile: ceil(S / 128) strips; the lanes of the last strip's two site steps"""
    shape = {name: (-(-kw['S'] // 128), min(64, (kw['S'] - 1) % 128 + 1), max(0, (kw['S'] - 1) % 128 + 1 - 64)) for name, kw in GC.STRIPS.items()}
    assert shape == {'N5-S300-gaps': (3, 44, 0), 'N12-S600-gaps': (5, 64, 24), 'N12-S200-generic': (2, 64, 8), 'N12-S300-C16': (3, 44, 0),
                     'N12-S130': (2, 2, 0), 'N12-S66': (1, 64, 2), 'N12-S128': (1, 64, 64)}
    assert GC.MIXTURES['C16'][0].size == 16 and GC.MIXTURES['C5'][0].size == 5 and GC.MIXTURES['C5'][0][0] == 0.0


# ---- B. 129 to 512 taxa: the site values stay clear of the floor under the mixtures -----------------------------------------------
@pytest.mark.parametrize("name", list(EC.BIG))
def test_big_cases_stay_roomy_under_the_mixtures(name):
    """every m of all five trees, by ordinary matrix products (no fma chain): under MIX_I_G4, and under C16 where the device runs it"""
    g, child, blen, Q = EC.big_case(name)
    for mix in [MIX_I_G4] + ([GC.C16] if name in ('generic-balanced-N512', 'caterpillar-N512') else []):
        worst = min(plain_site_values(c, b, Q, PRIOR, g, *mix).min() for c, b in zip(child, blen))
        print("%s under %d categories: smallest site value 2^%.1f" % (name, mix[0].size, np.log2(worst)))
        assert worst >= ROOMY


def test_strided_set_stays_roomy():
    """part C's sample of the 131 trees of 512 taxa, one category of rate 1: the plain site factors"""
    one = (np.array([1.0]), np.array([1.0]))
    for mixed in (False, True):
        g, child, blen, Q = EC.large_strided(mixed)
        assert child.shape[0] == 131 and g.shape[:2] == (512, 65)
        for t in (0, 1, 127, 128, 129, 130):
            assert plain_site_values(child[t], blen[t], Q, PRIOR, g, *one).min() >= ROOMY
        for w in range(128, 131):
            assert (child[w].tobytes() != child[w - 128].tobytes()) == mixed
    assert EC.updown_cap(512, 256) == 128 and EC.updown_cap(512, 304) == 128


# ---- B, C. the restatements at 50 digits on deep trees -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measured(name):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    return GC.measure_rates_big(mp, name), GC.measure_model_big(mp, name)


@pytest.mark.parametrize("name", GC.MP_CASES)
def test_reference_against_mpmath_big(name):
    """tree 0 of the case at four sites (the first, two variable ones, the last).  Measured: see treegrad_edges_cases.py."""
    rates, model = measured(name)
    print("%s: restatements against 50 digits, units of (scale + |value|) 2^-53: rates %r (E_REF_RATES_BIG = %g), model %r "
          "(E_REF_MODEL_BIG = %g)" % (name, rates, GC.E_REF_RATES_BIG, model, GC.E_REF_MODEL_BIG))
    assert max(rates[k] for k in ('grad', 'curv', 'drate', 'dweight')) <= GC.E_REF_RATES_BIG
    assert max(model.values()) <= GC.E_REF_MODEL_BIG


def test_big_bounds_are_not_stale():
    res = [measured(name) for name in GC.MP_CASES]
    worst_r = max(r[k] for r, _ in res for k in ('grad', 'curv', 'drate', 'dweight'))
    worst_m = max(max(m.values()) for _, m in res)
    assert GC.E_REF_RATES_BIG / 2 < worst_r <= GC.E_REF_RATES_BIG and GC.E_REF_MODEL_BIG / 2 < worst_m <= GC.E_REF_MODEL_BIG
    # deep trees need the wider bound under rate mixtures; the model call keeps the tolerance of the small trees
    assert GC.E_REF_RATES_BIG > E_REF_RATES and GC.TOL_RATES_BIG == 8 * GC.E_REF_RATES_BIG * UNIT
    assert GC.E_REF_MODEL_BIG <= E_REF_MODEL and GC.TOL_MODEL_BIG == TOL_MODEL
    # the subnormal category factor that the raw figures of caterpillar-N512 show (treegrad_edges_cases.py)
    cat = res[GC.MP_CASES.index('caterpillar-N512')][0]
    assert cat['subnormal_f'] >= 1 and cat['dweight_raw'] > 100 * cat['dweight']


# ---- D. the floor: the rate call ---------------------------------------------------------------------------------------------------
MIXES = {'I+G4': MIX_I_G4, 'slow-fast': GC.MIX_SLOW_FAST}
KEYS = (('grad', 'scale'), ('curv', 'scale'), ('drate', 'drate_scale'), ('dweight', 'dweight'))


@functools.lru_cache(maxsize=None)
def rates_base(mix):
    g, child, blen, Q = EC.scaled_base()
    rates, weights = MIXES[mix]
    M = np.array([category_matrices(Q, b, rates) for b in blen])          # fixed: the scaled alignments see the same matrices
    ref0 = TRR.trees_grad_rates(child, M, Q, PRIOR, g, blen, rates, weights)
    assert np.isfinite(ref0['loglik']).all() and (ref0['m'] > 2.0 ** -200).all()
    return g, child, blen, Q, M, ref0


@functools.lru_cache(maxsize=None)
def rates_scaled(place, mix):
    g, child, blen, Q, M, ref0 = rates_base(mix)
    e = EC.scaled_exponents(place, ref0['m'])
    return e, TRR.trees_grad_rates(child, M, Q, PRIOR, EC.scaled_leaves(g, e), blen, *MIXES[mix])


def units(ref, ref0, k, sk):
    with np.errstate(invalid='ignore'):
        return np.nanmax(np.abs(ref[k] - ref0[k]) / ((ref0[sk] + np.abs(ref0[k])) * UNIT))


@pytest.mark.parametrize("place,mix", [(p, 'I+G4') for p in EC.PLACES] + [(p, 'slow-fast') for p in EC.IN_RANGE])
def test_rates_reference_on_the_scaled_cases(place, mix):
    """what test_gpu_treegrad_rates_edges.py asks of the device, asked of the restatement first"""
    g, child, blen, Q, M, ref0 = rates_base(mix)
    e, ref = rates_scaled(place, mix)
    m, f = ref['m'][:, AT], ref['f'][:, :, AT]
    sub = int(((f > 0) & (f < 2.0 ** -1022)).sum())
    print(place, mix, "scaled site values in [2^%.1f, 2^%.1f], %d subnormal category factors"
          % (np.log2(max(m.min(), 5e-324)), np.log2(max(m.max(), 5e-324)), sub))
    np.testing.assert_array_equal(np.delete(ref['m'], AT, axis=1), np.delete(ref0['m'], AT, axis=1))
    if place == '2^-900':
        assert (m < 2.0 ** -880).all() and (m > 2.0 ** -960).all() and sub == 0
        for k, _ in KEYS:
            np.testing.assert_array_equal(bits(ref[k]), bits(ref0[k]), err_msg=k)
        np.testing.assert_allclose(ref['loglik'], ref0['loglik'] - e.sum() * np.log(2.0), rtol=1e-12, atol=0)
    elif place in EC.IN_RANGE:
        assert (m >= FLOOR).all() and (m <= ROOMY).all()
        if place == 'at-the-floor':
            assert (m.min(axis=0) < 2.0 ** -1019).all() and sub >= 1
        for k, sk in KEYS:
            assert np.isfinite(ref[k]).all()
        assert units(ref, ref0, 'grad', 'scale') * UNIT <= TOL_RATES and units(ref, ref0, 'curv', 'scale') * UNIT <= TOL_RATES
    else:
        assert (m < FLOOR).all() and all(np.isnan(ref[k]).all() for k, _ in KEYS)
        if place == 'just-below':
            assert (m.max(axis=0) >= 2.0 ** -1021).all()
        if place == 'zero':
            assert (m == 0).all() and (ref['loglik'] == -np.inf).all()
        else:
            assert (m > 0).all() and np.isfinite(ref['loglik']).all()


def test_the_finding_is_inside_its_bound_and_outside_the_plain_tolerance():
    """drate and dweight of the restatement, scaled against unscaled: inside TOL_RATES (scale + |value|) + floor_excess at every
    in-range place under both mixtures; at-the-floor under MIX_I_G4 far outside TOL_RATES alone, with subnormal category factors
    beside site values in range -- without which the device test of the bound would ask nothing"""
    worst = 0.0
    for mix in MIXES:
        g, child, blen, Q, M, ref0 = rates_base(mix)
        for place in EC.IN_RANGE:
            _, ref = rates_scaled(place, mix)
            ex_r, ex_w = GC.floor_excess(ref['m'][:, AT], blen, MIXES[mix][1])
            assert (ex_r >= 0).all() and (ex_w > 0).all() and np.isfinite(ex_r).all() and np.isfinite(ex_w).all()
            a = GC.close_with_excess("%s %s drate" % (place, mix), ref['drate'], ref0['drate'], ref0['drate_scale'], ex_r)
            b = GC.close_with_excess("%s %s dweight" % (place, mix), ref['dweight'], ref0['dweight'], ref0['dweight'], ex_w)
            worst = max(worst, a, b)
    print("worst ratio to the bound %.3f (WORST_RATIO = %g)" % (worst, GC.WORST_RATIO))
    assert GC.WORST_RATIO / 2 < worst <= GC.WORST_RATIO
    _, ref0 = rates_base('I+G4')[4:]
    _, ref = rates_scaled('at-the-floor', 'I+G4')
    f, m = ref['f'][:, :, AT], ref['m'][:, AT]
    dr, dw = units(ref, ref0, 'drate', 'drate_scale'), units(ref, ref0, 'dweight', 'dweight')
    print("at-the-floor under +I+G4, plain units: drate %.3g, dweight %.3g (TOL_RATES: %.3g)" % (dr, dw, TOL_RATES / UNIT))
    assert dr > 10 * TOL_RATES / UNIT and dw > 100 * TOL_RATES / UNIT     # measured: 3.7e3 and 9.8e4 beside 61
    assert ((f > 0) & (f < 2.0 ** -1022)).sum() >= 1 and (m >= FLOOR).all()
    assert GC.K_W == 5 and GC.K_R == 35


def test_hardware_fma_is_the_emulation_in_range_and_the_bound_holds_with_it():
    """treegrad_edges_cases.hardware_fma, under which the device file restates the scaled alignments: on the unscaled alignment
    and at 2^-900 it changes no bit; at the floor it moves the subnormal category factors, and drate and dweight stay inside
    the near-floor bound against the unscaled restatement as they do under the emulation"""
    g, child, blen, Q, M, ref0 = rates_base('I+G4')
    with GC.hardware_fma():
        again = TRR.trees_grad_rates(child, M, Q, PRIOR, g, blen, *MIX_I_G4)
        e900 = EC.scaled_exponents('2^-900', ref0['m'])
        far = TRR.trees_grad_rates(child, M, Q, PRIOR, EC.scaled_leaves(g, e900), blen, *MIX_I_G4)
        e = EC.scaled_exponents('at-the-floor', ref0['m'])
        near = TRR.trees_grad_rates(child, M, Q, PRIOR, EC.scaled_leaves(g, e), blen, *MIX_I_G4)
    assert TR.fma.__module__ == 'treegrad_ref'                            # the context put the emulation back
    for k in ('loglik', 'grad', 'curv', 'drate', 'dweight', 'm', 'f'):
        np.testing.assert_array_equal(bits(again[k]), bits(ref0[k]), err_msg=k)
        np.testing.assert_array_equal(bits(far[k]), bits(rates_scaled('2^-900', 'I+G4')[1][k]), err_msg=k)
    emulated = rates_scaled('at-the-floor', 'I+G4')[1]
    np.testing.assert_array_equal(bits(near['m']), bits(emulated['m']))   # the site values: rates_ref.mix is exact either way ...
    moved = (bits(near['f']) != bits(emulated['f'])).sum()
    print("at the floor: %d category factors differ between the emulated and the hardware fma" % moved)
    assert moved >= 1                                                     # ... the subnormal factors are not
    ex_r, ex_w = GC.floor_excess(near['m'][:, AT], blen, MIX_I_G4[1])
    GC.close_with_excess("hardware fma, drate", near['drate'], ref0['drate'], ref0['drate_scale'], ex_r)
    GC.close_with_excess("hardware fma, dweight", near['dweight'], ref0['dweight'], ref0['dweight'], ex_w)
    assert units(near, ref0, 'grad', 'scale') * UNIT <= TOL_RATES and units(near, ref0, 'curv', 'scale') * UNIT <= TOL_RATES


def test_rates_one_site_below_the_floor():
    """the trees that stay in range keep grad and curv within TOL_RATES (measured: 0 units).  Their site value at the scaled site
    lies just above the floor, so drate and dweight are the finding again (measured: drate 763 units of plain TOL_RATES' scale):
    they are held to the near-floor bound with that one site's excess, and the device test does the same"""
    g, child, blen, Q, M, ref0 = rates_base('I+G4')
    gs = GC.scale_one_site(g, GC.one_site_below(ref0['m']))
    ref = TRR.trees_grad_rates(child, M, Q, PRIOR, gs, blen, *MIX_I_G4)
    out = (ref['m'] < FLOOR).any(axis=1)
    assert 1 <= out.sum() < out.size and (ref['m'] > 0).all() and np.isfinite(ref['loglik']).all()
    assert (ref['m'][~out, 129] < ROOMY).all()
    for k, sk in KEYS:
        assert np.isnan(ref[k][out]).all()
        with np.errstate(invalid='ignore'):
            err = np.abs(ref[k][~out] - ref0[k][~out]) / (ref0[sk][~out] + np.abs(ref0[k][~out]))
        print("in-range trees, %s: %.3g units" % (k, np.nanmax(err) / UNIT))
        if k in ('grad', 'curv'):
            assert (err <= TOL_RATES).all(), k
    ex_r, ex_w = GC.floor_excess(ref['m'][~out][:, [129]], blen[~out], MIX_I_G4[1])
    GC.close_with_excess("in-range trees, drate", ref['drate'][~out], ref0['drate'][~out], ref0['drate_scale'][~out], ex_r)
    GC.close_with_excess("in-range trees, dweight", ref['dweight'][~out], ref0['dweight'][~out], ref0['dweight'][~out], ex_w)


# ---- D. the floor: the model call --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_base():
    g, child, blen, Q = EC.scaled_base()
    dirs = GC.model_directions(12, Q)
    M = branch_matrices(Q, blen)
    D = MR.direction_matrices(Q, dirs, blen)
    ref0 = MR.trees_grad_model(child, M, D, PRIOR, g, tile=64)
    grad0 = TR.trees_grad(child, M, Q, PRIOR, g, want_sites=True)
    assert np.isfinite(ref0[0]).all() and (grad0[4] > 2.0 ** -200).all()
    return g, child, M, D, Q, ref0, grad0


def within(got, ref, scale, tol):
    return (np.abs(got - ref) <= tol * (scale + np.abs(ref))).all()


@pytest.mark.parametrize("place", EC.PLACES)
def test_model_reference_on_the_scaled_cases(place):
    g, child, M, D, Q, (ll0, dth0, dpr0, sc_t, sc_p), (_, grad0, _, sc_g, L0) = model_base()
    e = EC.scaled_exponents(place, L0)
    gs = EC.scaled_leaves(g, e)
    ll, dth, dpr, _, _ = MR.trees_grad_model(child, M, D, PRIOR, gs, tile=64)
    _, grad, _, _, L = TR.trees_grad(child, M, Q, PRIOR, gs, want_sites=True)
    if place == '2^-900':
        assert (L[:, AT] < 2.0 ** -880).all() and (L[:, AT] > 2.0 ** -960).all()
        for a, a0 in ((dth, dth0), (dpr, dpr0), (grad, grad0)):
            np.testing.assert_array_equal(bits(a), bits(a0))
        np.testing.assert_allclose(ll, ll0 - e.sum() * np.log(2.0), rtol=1e-12, atol=0)
    elif place in EC.IN_RANGE:
        assert (L[:, AT] >= FLOOR).all() and (L[:, AT] <= ROOMY).all()
        if place == 'at-the-floor':
            assert (L[:, AT].min(axis=0) < 2.0 ** -1019).all()
        assert within(dth, dth0, sc_t, TOL_MODEL) and within(dpr, dpr0, sc_p, TOL_MODEL) and within(grad, grad0, sc_g, TOL_MODEL)
    else:
        assert (L[:, AT] < FLOOR).all() and np.isnan(dth).all() and np.isnan(dpr).all() and np.isnan(grad).all()
        if place == 'just-below':
            assert (L[:, AT].max(axis=0) >= 2.0 ** -1021).all()
        assert (ll == -np.inf).all() if place == 'zero' else np.isfinite(ll).all()


def test_model_one_site_below_the_floor():
    g, child, M, D, Q, (ll0, dth0, dpr0, sc_t, sc_p), (_, grad0, _, sc_g, L0) = model_base()
    gs = GC.scale_one_site(g, GC.one_site_below(L0))
    ll, dth, dpr, _, _ = MR.trees_grad_model(child, M, D, PRIOR, gs, tile=64)
    L = TR.trees_site_factors(child, M, PRIOR, gs)
    out = (L < FLOOR).any(axis=1)
    assert 1 <= out.sum() < out.size and (L > 0).all() and np.isfinite(ll).all()
    assert np.isnan(dth[out]).all() and np.isnan(dpr[out]).all()
    assert within(dth[~out], dth0[~out], sc_t[~out], TOL_MODEL) and within(dpr[~out], dpr0[~out], sc_p[~out], TOL_MODEL)
