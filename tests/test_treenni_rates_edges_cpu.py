"""The edges of phylo_trees_nni_rates without a GPU (inputs: treenni_rates_edges_cases.py,
treegrad_edges_cases.py, trees_edges_cases.py): the restatement against the same formulas at 50 digits on trees of 129 to 512 taxa
under genuine mixtures (E_NNI_RATES_BIG, E_EXPL_RATES_BIG), the C-dependent grid cap against ptnr_make_plan itself, and every
precondition that test_gpu_treenni_rates_edges.py asserts again before it compares anything: zero-length branches of the strip
cases, site values clear of the floor under the mixtures, the NaN and -inf patterns of the big cases, the invariant class at
variable sites, the sets of a workgroup's second item, the places of the scaled sites with the near-floor contract of delta, and
the random columns that reach the floor between 390 and 400 taxa."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import treegrad_edges_cases as GC
import treegrad_ref as TR
import treenni_rates_edges_cases as XC
import trees_edges_cases as EC
from test_gpu_treenni_rates import missing_moves
from test_gpu_trees_loglik import alignment, bits, gtr_Q, random_trees
from treegrad_rates_cases import MIX_I_G4, plain_site_values
from treenni_rates_cases import E_EXPL_RATES, E_NNI_RATES, TOL_EXPL_RATES, TOL_NNI_RATES, tree_category_matrices
from trees_edges_cases import FLOOR, PRIOR, ROOMY

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
AT = list(EC.SCALED_SITES)
UNIT = 2.0 ** -53


# ---- A. the strip cases --------------------------------------------------------------------------------------------------------------
def test_strip_cases():
    """treegrad_edges_cases.STRIPS as they stand (their strips and lanes: test_treegrad_edges_cpu.py): seven random trees with
    zero-length branches and every m far above the floor (no move of these sets is impossible: the -inf entries that the device
    file compares are those of the big cases)"""
    assert list(GC.STRIPS) == ['N5-S300-gaps', 'N12-S600-gaps', 'N12-S200-generic', 'N12-S300-C16', 'N12-S130', 'N12-S66', 'N12-S128']
    assert max(-(-kw['S'] // 128) for kw in GC.STRIPS.values()) == 5
    for name, kw in GC.STRIPS.items():
        N, S = kw['N'], kw['S']
        rates, weights = GC.MIXTURES[kw['mix']]
        g = alignment(N, S, 100 + N + S, kw.get('gaps', False), kw.get('generic', False))
        child, blen = random_trees(N, 5, XC.T_STRIPS)
        assert child.shape[0] == 7 and (blen == 0).any()
        ll, delta, absd, m = XC.restated(child, tree_category_matrices(gtr_Q(), blen, rates), PRIOR, g, rates, weights)
        assert np.isfinite(ll).all() and (m > 2.0 ** -200).all()
        np.testing.assert_array_equal(np.isnan(delta), missing_moves(child))
        print("%s: %d -inf, %d NaN" % (name, np.isneginf(delta).sum(), np.isnan(delta).sum()))
        assert not np.isneginf(delta).any()


# ---- B. 129 to 512 taxa: what the device test takes for granted ----------------------------------------------------------------------
def big_preconditions(name, mix, trees):
    kw = EC.BIG[name]
    g, child, blen, Q = EC.big_case(name)
    child, blen = child[trees], blen[trees]
    rates, weights = mix
    M = tree_category_matrices(Q, blen, rates)
    ll, delta, absd, m = XC.restated(child, M, PRIOR, g, rates, weights, exact_mix=False)
    print("%s C%d: site values in [2^%.1f, 2^%.1f], %d -inf, %d NaN" % (name, rates.size, np.log2(m.min()), np.log2(m.max()),
                                                                     np.isneginf(delta).sum(), np.isnan(delta).sum()))
    assert (m >= ROOMY).all() and np.isfinite(m).all() and np.isfinite(ll).all()
    miss = missing_moves(child)
    np.testing.assert_array_equal(np.isnan(delta), miss)
    assert (np.isfinite(delta) | np.isneginf(delta))[~miss].all() and not miss[:, :-1].any()
    if kw['shape'] == 'balanced':
        assert not np.isneginf(delta).any() and not miss.any()
    elif kw['shape'] == 'caterpillar':
        assert np.isneginf(delta).any() and miss[:, -1].all()             # impossible neighbours; a leaf at the root kills the root row
    assert rates[0] == 0.0                                                # the invariant class: f_0 = 0 exactly at the variable sites
    f0 = TR.site_factors(child[0], M[0, 0], PRIOR, g)
    direct = (PRIOR * g.prod(axis=0)).sum(axis=-1)
    np.testing.assert_array_equal(f0 == 0, direct == 0)
    assert (f0 == 0).any()


@pytest.mark.parametrize("name", list(EC.BIG))
def test_many_taxa_cases(name):
    """all five trees at 129 and 257 taxa; at 512 the generating tree and one neighbour (the device file asserts the same of all
    five, at four seconds of restatement a tree)"""
    big_preconditions(name, MIX_I_G4, slice(None) if EC.BIG[name]['N'] < 512 else [0, 2])


@pytest.mark.parametrize("name", ['caterpillar-N512', 'generic-balanced-N512'])
def test_512_taxa_16_categories_cases(name):
    assert GC.C16[0].size == 16 and len(set(GC.C16[0].tolist())) == 16 and (GC.C16[1] > 0).all()      # sixteen different planes, all weighted
    big_preconditions(name, GC.C16, [0, 2])


def test_two_strip_case():
    g, child, blen, Q = EC.two_strip_case()
    rates, weights = MIX_I_G4
    assert g.shape[:2] == (257, 200)
    ll, delta, absd, m = XC.restated(child[[0, 2]], tree_category_matrices(Q, blen[[0, 2]], rates), PRIOR, g, rates, weights, exact_mix=False)
    for c, b in zip(child, blen):
        assert plain_site_values(c, b, Q, PRIOR, g, rates, weights).min() >= ROOMY
    assert (m >= ROOMY).all() and np.isfinite(ll).all() and not np.isnan(delta).any() and not np.isneginf(delta).any()


def test_per_tree_mixtures_at_depth():
    """random-N257 under five different +I+G4 mixtures: every one keeps every m of its tree clear of the floor"""
    g, child, blen, Q = EC.big_case('random-N257')
    rt, wt = XC.per_tree_mixtures()
    assert rt.shape == wt.shape == (5, 5) and len({r.tobytes() for r in rt}) == 5 and (rt[:, 0] == 0).all() and (wt[:, 0] > 0).all()
    for t in range(5):
        assert plain_site_values(child[t], blen[t], Q, PRIOR, g, rt[t], wt[t]).min() >= ROOMY


# ---- B. the restatement at 50 digits on deep trees under mixtures: E_NNI_RATES_BIG, E_EXPL_RATES_BIG -------------------------------
@functools.lru_cache(maxsize=None)
def measured(name, mix):
    mp = pytest.importorskip("mpmath")
    g, child, blen, Q = EC.big_case(name)
    if mix == 'C16':
        case, trees, S = XC.MP_C16
        assert case == name
        return XC.measure_deep_rates(mp, child[list(trees)], blen[list(trees)], Q, PRIOR, g[:, :S], *GC.C16)
    trees = list(XC.MP_TREES)
    return XC.measure_deep_rates(mp, child[trees], blen[trees], Q, PRIOR, g[:, :XC.S_MP], *MIX_I_G4)


MP_RUNS = [(name, 'I+G4') for name in XC.MP_CASES] + [(XC.MP_C16[0], 'C16')]


@pytest.mark.parametrize("name,mix", MP_RUNS, ids=['%s-%s' % r for r in MP_RUNS])
def test_reference_against_mpmath_big(name, mix):
    """Trees 0 and 2 of the case at the first six sites under MIX_I_G4 (tree 0 at three sites under C16): delta over EVERY move,
    the explicit comparison over treenni_cases.move_sample.  Measured: see treenni_rates_edges_cases.py."""
    worst_n, worst_x, seen, dead = measured(name, mix)
    print("%s %s: restatement against 50 digits over %d moves (%d impossible): delta %.3f units (E_NNI_RATES_BIG = %g), explicit "
          "neighbours %.3f units (E_EXPL_RATES_BIG = %g)" % (name, mix, seen, dead, worst_n, XC.E_NNI_RATES_BIG, worst_x, XC.E_EXPL_RATES_BIG))
    N = EC.BIG[name]['N']
    assert seen >= (1 if mix == 'C16' else 2) * 2 * (N - 2)
    if EC.BIG[name]['shape'] == 'caterpillar':
        assert dead >= 1
    assert worst_n <= XC.E_NNI_RATES_BIG
    assert worst_x <= XC.E_EXPL_RATES_BIG


def test_big_bounds_are_not_stale():
    """over the whole set the worst errors lie above half the bounds: a constant left behind by a change of the cases fails"""
    res = [measured(*run) for run in MP_RUNS]
    worst_n, worst_x = max(r[0] for r in res), max(r[1] for r in res)
    print("over %d runs: delta %.3f units (E_NNI_RATES_BIG = %g), explicit neighbours %.3f units (E_EXPL_RATES_BIG = %g)"
          % (len(res), worst_n, XC.E_NNI_RATES_BIG, worst_x, XC.E_EXPL_RATES_BIG))
    assert XC.E_NNI_RATES_BIG / 2 < worst_n <= XC.E_NNI_RATES_BIG
    assert XC.E_EXPL_RATES_BIG / 2 < worst_x <= XC.E_EXPL_RATES_BIG
    assert XC.TOL_NNI_RATES_BIG == 8 * max(E_NNI_RATES, XC.E_NNI_RATES_BIG) * UNIT
    assert XC.TOL_EXPL_RATES_BIG == 8 * max(E_EXPL_RATES, XC.E_EXPL_RATES_BIG) * UNIT
    assert XC.E_NNI_RATES_BIG > E_NNI_RATES                               # deep trees need the wider bound ...
    assert XC.TOL_EXPL_RATES_BIG == TOL_EXPL_RATES                        # ... the explicit comparison keeps that of the small trees


# ---- C. a workgroup's second item ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_program():
    """tests/treenni_rates_asan_main.cpp, which prints ptnr_make_plan's chunk and grid when it gets a call's shape"""
    import tempfile
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tempfile.mkdtemp(prefix="treenni_rates_plan"), "plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "phylo_amd", "csrc"),
                           os.path.join(ROOT, "tests", "treenni_rates_asan_main.cpp"), "-o", exe])
    return exe


def plan(N, ntiles, T, C, coded, cus):
    out = subprocess.run([plan_program()] + [str(int(v)) for v in (N, ntiles, T, C, coded, cus)], stdout=subprocess.PIPE, timeout=60, check=True)
    w = out.stdout.decode().split()
    return {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}


def test_rates_cap_is_the_plans():
    """rates_cap against ptnr_make_plan (the host half of the header, compiled here): the grid of a call with more items than the
    cap IS the cap, at every N, C and number of compute units tried; the two sets of part C go in one chunk each"""
    for cus in (64, 256, 304):
        assert XC.rates_cap(512, 5, cus) == 25 and XC.rates_cap(512, 16, cus) == 8
        assert XC.rates_cap(5, 2, cus) == 8 * cus == EC.updown_cap(5, cus) and XC.rates_cap(512, 1, cus) == EC.updown_cap(512, cus)
        for N, C in ((512, 5), (512, 16), (257, 5), (129, 16), (5, 2), (12, 16)):
            assert plan(N, 3, 4096, C, 1, cus)['grid'] == XC.rates_cap(N, C, cus), (N, C, cus)
        for C, T in XC.T_SECOND.items():
            p = plan(512, 1, T, C, 1, cus)
            assert p['chunk'] == T and p['grid'] == XC.rates_cap(512, C, cus) == T - 3 and T * p['per_tree'] < (64 << 20)
    assert plan(512, 1, 28, 5, 1, 256)['per_tree'] < 1 << 20              # "about 0.9 MB a tree"


def test_second_item_sets_stay_roomy():
    """both sets of part C: the sampled trees keep every m above ROOMY, and one workgroup's two items differ in topology"""
    for C, mix in ((5, MIX_I_G4), (16, GC.C16)):
        T, cap = XC.T_SECOND[C], XC.rates_cap(512, C, 256)
        g, child, blen, Q = EC.large_strided(True, T)
        assert child.shape == (T, 511, 2) and g.shape[:2] == (512, 65) and T == cap + 3
        for w in range(cap, T):
            assert child[w].tobytes() != child[w - cap].tobytes()
        assert XC.SAMPLE_SECOND[C][-3:] == list(range(cap, T)) and XC.SAMPLE_SECOND[C][0] == 0
        for t in XC.SAMPLE_SECOND[C]:
            assert plain_site_values(child[t], blen[t], Q, PRIOR, g, *mix).min() >= ROOMY


# ---- D. the floor of the range, on the mixed site value m ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def floor_base(mix):
    g, child, blen, Q = EC.scaled_base()
    rates, weights = XC.FLOOR_MIXES[mix]
    M = tree_category_matrices(Q, blen, rates)                            # fixed: the scaled alignments see the same matrices
    ref0 = XC.restated(child, M, PRIOR, g, rates, weights)
    assert np.isfinite(ref0[0]).all() and (ref0[3] > 2.0 ** -200).all()
    return g, child, M, ref0


@functools.lru_cache(maxsize=None)
def floor_scaled(place, mix, hardware):
    g, child, M, (ll0, delta0, absd0, m0) = floor_base(mix)
    rates, weights = XC.FLOOR_MIXES[mix]
    gs = EC.scaled_leaves(g, EC.scaled_exponents(place, m0))
    if hardware:
        with GC.hardware_fma():
            return XC.restated(child, M, PRIOR, gs, rates, weights), [XC.tree_values(c, mm, PRIOR, gs, weights) for c, mm in zip(child, M)]
    return XC.restated(child, M, PRIOR, gs, rates, weights), [XC.tree_values(c, mm, PRIOR, gs, weights) for c, mm in zip(child, M)]


@pytest.mark.parametrize("place,mix", [(p, 'I+G4') for p in EC.PLACES] + [(p, 'slow-fast') for p in EC.IN_RANGE])
def test_reference_on_the_scaled_cases(place, mix):
    """what test_gpu_treenni_rates_edges.py asks of the device, asked of the restatement first (under the emulated fma and under
    hardware_fma, which the device file uses on the scaled alignments)"""
    g, child, M, (ll0, delta0, absd0, m0) = floor_base(mix)
    miss = missing_moves(child)
    np.testing.assert_array_equal(np.isnan(delta0), miss)
    e = EC.scaled_exponents(place, m0)
    S = g.shape[1]
    for hardware in (False, True):
        (ll, delta, absd, m), vals = floor_scaled(place, mix, hardware)
        ms = m[:, AT]
        fp = np.array([v[:, AT] for val in vals for v in val[3].values()])        # every neighbour's category factors at the scaled sites
        f = np.array([val[1][:, AT] for val in vals])
        sub = int(((fp > 0) & (fp < 2.0 ** -1022)).sum())
        print(place, mix, "hardware fma" if hardware else "emulated fma", "scaled site values in [2^%.1f, 2^%.1f], %d subnormal category "
              "factors of neighbours" % (np.log2(max(ms.min(), 5e-324)), np.log2(max(ms.max(), 5e-324)), sub))
        np.testing.assert_array_equal(bits(np.delete(m, AT, axis=1)), bits(np.delete(m0, AT, axis=1)))
        if place in EC.IN_RANGE:
            assert (ms >= FLOOR).all() and (ms <= (2.0 ** -880 if place == '2^-900' else ROOMY)).all() and np.isfinite(ll).all()
            np.testing.assert_allclose(ll, ll0 - e.sum() * np.log(2.0), rtol=1e-12, atol=0)
            np.testing.assert_array_equal(np.isnan(delta), miss)
            np.testing.assert_array_equal(np.isneginf(delta), np.isneginf(delta0))
            if place == '2^-900':
                assert ((fp == 0) | (fp >= 2.0 ** -1022)).all() and ((f == 0) | (f >= 2.0 ** -1022)).all()    # every positive factor is normal
            if place == 'at-the-floor':
                assert (ms.min(axis=0) < 2.0 ** -1019).all() and sub >= 1
            if place in ('2^-900', 'inside'):
                np.testing.assert_array_equal(bits(delta), bits(delta0))
            fin = np.isfinite(delta0)
            assert (np.abs(delta - delta0)[fin] <= TOL_NNI_RATES * (S + absd0[fin] + np.abs(delta0[fin]))).all()
        else:
            assert (ms < FLOOR).all() and np.isnan(delta).all()
            if place == 'just-below':
                assert (ms.max(axis=0) >= 2.0 ** -1021).all()
            if place == 'zero':
                assert (ms == 0).all() and (ll == -np.inf).all()
            else:
                assert (ms > 0).all() and np.isfinite(ll).all()


def test_near_floor_contract():
    """delta of the restatement, scaled against unscaled, at every in-range place under both mixtures and both fma: inside the
    counted allowance sum_s K_NNI C_live 2^-1075 / m'_s move by move (worst ratio FLOOR_WORST_RATIO), and -- what decides the
    device test -- inside plain TOL_NNI_RATES by two orders of magnitude (FLOOR_PLAIN_UNITS of its 23.2 units): no allowance is
    used on the device.  The subnormal factors and a neighbour's m' below 2^-1020 are there (asserted), or this would ask nothing."""
    worst_ratio = worst_units = 0.0
    smallest, moved = 1.0, 0
    for mix, (rates, weights) in XC.FLOOR_MIXES.items():
        g, child, M, (ll0, delta0, absd0, m0) = floor_base(mix)
        S = g.shape[1]
        c_live = int((weights > 0).sum())
        for place in EC.IN_RANGE:
            for hardware in (False, True):
                (ll, delta, absd, m), vals = floor_scaled(place, mix, hardware)
                for t, val in enumerate(vals):
                    for key, mp in val[2].items():
                        if not np.isfinite(delta0[t][key]):
                            continue
                        diff = abs(delta[t][key] - delta0[t][key])
                        moved += diff > 0
                        smallest = min(smallest, mp[AT].min())
                        worst_ratio = max(worst_ratio, diff / XC.floor_allowance(mp[AT], c_live))
                        worst_units = max(worst_units, diff / ((S + absd0[t][key] + abs(delta0[t][key])) * UNIT))
    print("near the floor: worst |scaled - unscaled| / allowance %.3f (FLOOR_WORST_RATIO = %g); the same differences in plain units %.3f "
          "(FLOOR_PLAIN_UNITS = %g; TOL_NNI_RATES is %.1f); %d entries moved; smallest m' 2^%.1f"
          % (worst_ratio, XC.FLOOR_WORST_RATIO, worst_units, XC.FLOOR_PLAIN_UNITS, TOL_NNI_RATES / UNIT, moved, np.log2(smallest)))
    assert XC.FLOOR_WORST_RATIO / 2 < worst_ratio <= XC.FLOOR_WORST_RATIO
    assert XC.FLOOR_PLAIN_UNITS / 2 < worst_units <= XC.FLOOR_PLAIN_UNITS
    assert 100 * XC.FLOOR_PLAIN_UNITS < TOL_NNI_RATES / UNIT              # why the device test needs no allowance
    assert moved >= 1 and 0 < smallest < FLOOR and XC.K_NNI == 28


def test_hardware_fma_changes_nothing_in_range():
    """under hardware_fma the unscaled alignment and the one scaled to 2^-900 keep the emulation's bits"""
    g, child, M, ref0 = floor_base('I+G4')
    with GC.hardware_fma():
        again = XC.restated(child, M, PRIOR, g, *MIX_I_G4)
    assert TR.fma.__module__ == 'treegrad_ref'                            # the context put the emulation back
    for a, b in zip(again, ref0):
        np.testing.assert_array_equal(bits(a), bits(b))
    for a, b in zip(floor_scaled('2^-900', 'I+G4', True)[0], floor_scaled('2^-900', 'I+G4', False)[0]):
        np.testing.assert_array_equal(bits(a), bits(b))


# ---- D. coded leaves: random columns between 300 and 400 taxa ------------------------------------------------------------------------
def test_random_columns_reach_the_floor_at_400_taxa():
    """the search of treenni_rates_edges_cases.py's last section, by ordinary matrix products: N = 400 is the smallest N of 300,
    310, ... 400 at which tree 0 has an m below the floor under MIX_I_G4, and none is zero.  Then the two device cases by the
    restatement: at 390 taxa trees 0 and 1 stay in range (tree 0 with values below ROOMY) and tree 2 leaves it; at 400 all do."""
    first = None
    for N in range(300, 401, 10):
        g, child, blen, Q = EC.random_columns(N)
        m = plain_site_values(child[0], blen[0], Q, PRIOR, g, *MIX_I_G4)
        if (m < FLOOR).any() and (m > 0).all():
            first = N
            break
        assert (m >= FLOOR).all(), N
    assert first == XC.N_COLUMNS_OUT == 400 and XC.N_COLUMNS_IN == 390
    rates, weights = MIX_I_G4
    for N in (XC.N_COLUMNS_IN, XC.N_COLUMNS_OUT):
        g, child, blen, Q = EC.random_columns(N)
        with GC.hardware_fma():
            ll, delta, absd, m = XC.restated(child, tree_category_matrices(Q, blen, rates), PRIOR, g, rates, weights)
        out = (m < FLOOR).any(axis=1)
        print("N = %d: smallest m per tree 2^%s, values below the floor %s" % (N, np.log2(m.min(axis=1)).round(1), (m < FLOOR).sum(axis=1)))
        assert (m > 0).all() and np.isfinite(ll).all() and np.isnan(delta[out]).all()
        np.testing.assert_array_equal(np.isnan(delta[~out]), missing_moves(child[~out]))
        if N == XC.N_COLUMNS_IN:
            assert out.tolist() == [False, False, True] and m[0].min() < ROOMY
        else:
            assert out.all()
