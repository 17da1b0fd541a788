"""Shared inputs and bounds of the edge tests of phylo_trees_nni_rates where its own suite stops: items of
several strips, 129 to 512 taxa under genuine mixtures, a workgroup's second 512-taxon item under 5 and 16 categories, the mixed
site value m at the floor of the double range.  The trees, alignments and places are those of trees_edges_cases.py, the strip
cases and mixtures those of treegrad_edges_cases.py; here are the restatement's error against 50 digits on deep trees under
mixtures, the C-dependent grid cap, and the near-floor bound of delta.  test_treenni_rates_edges_cpu.py holds every case to its
precondition from the NumPy restatement alone; test_gpu_treenni_rates_edges.py asserts them again before it compares anything."""
import numpy as np

import treegrad_edges_cases as GC
import treegrad_ref as TR
import treenni_cases as NC
import treenni_rates_cases as RC
import treenni_rates_ref as RR
import trees_edges_cases as EC
from phylo_amd import rates as R
from phylo_amd.treesearch import apply_nni, nni_moves
from treegrad_rates_cases import MIX_I_G4, category_matrices
from treenni_rates_cases import E_EXPL_RATES, E_NNI_RATES

PRIOR = EC.PRIOR
T_STRIPS = 7

# ---- B, C. the restatement against 50 digits above 128 taxa under mixtures --------------------------------------------------------
# Measured by test_treenni_rates_edges_cpu.py::test_reference_against_mpmath_big on trees 0 and 2 of MP_CASES at the first six
# sites of the case's alignment under MIX_I_G4 (p_inv 0.1 + Gamma4(0.5)), and on tree 0 of caterpillar-N512 at the first three
# sites under treegrad_edges_cases.C16 (+I+G15), in the units of test_treenni_rates_cpu.py::test_reference_against_mpmath: delta
# over EVERY move in (S + sum_s |d_s|) 2^-53, the explicit comparison over treenni_cases.move_sample in
# (S + sum_s |log m_s| + sum_s |log m'_s|) 2^-53.
#   MIX_I_G4             delta   explicit                                  C16                  delta   explicit
#   caterpillar-N129      5.00    1.60                                     caterpillar-N512     20.75   0.72
#   caterpillar-N257      8.12    1.12
#   caterpillar-N512     19.75    1.40
#   random-N257           3.30    1.38
#   balanced-N129         2.89    1.41
# 6124 moves, 39 of them impossible.  As in section 14 the error of delta grows with a caterpillar's depth (the plain call: 18.97
# at 512 taxa) and E_NNI_RATES = 2.9 does not cover it; the mixing chain adds little, and sixteen categories one unit more.  The
# explicit comparison stays below E_EXPL_RATES = 1.9, so TOL_EXPL_RATES_BIG is TOL_EXPL_RATES.
# test_treenni_rates_edges_cpu.py::test_big_bounds_are_not_stale keeps the worst at or below each bound and above half of it.
E_NNI_RATES_BIG = 21.0
E_EXPL_RATES_BIG = 1.7
TOL_NNI_RATES_BIG = 8 * max(E_NNI_RATES, E_NNI_RATES_BIG) * 2.0 ** -53
TOL_EXPL_RATES_BIG = 8 * max(E_EXPL_RATES, E_EXPL_RATES_BIG) * 2.0 ** -53
MP_CASES = ('caterpillar-N129', 'caterpillar-N257', 'caterpillar-N512', 'random-N257', 'balanced-N129')
MP_TREES = (0, 2)
S_MP = 6
MP_C16 = ('caterpillar-N512', (0,), 3)                                     # case, trees, sites under C16


def restated_loglik_rates(child, M, prior, g, weights, memo):
    """treenni_rates_ref.tree_loglik_sites' two numbers and bits, M [C][N-1][2][4][4], with the partial of every subtree met so far
    kept in memo per category as treenni_cases.restated_loglik keeps it: a neighbour costs the nodes above its move"""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    N = g.shape[0]
    R = N - 1
    f = []
    with np.errstate(all='ignore'):
        for c in range(w.size):
            ids, xs = memo.setdefault(('ids', c), {}), memo.setdefault(('x', c), {})
            at = list(range(N)) + [None] * R
            for i in range(R):
                kids = (at[child[i][0]], at[child[i][1]])
                key = (kids[0], M[c, i, 0].tobytes(), kids[1], M[c, i, 1].tobytes())
                me = ids.setdefault(key, N + len(ids))
                at[N + i] = me
                if me not in xs:
                    xk = [g[k] if k < N else xs[k] for k in kids]
                    xs[me] = NC._row_times4(xk[0], M[c, i, 0]) * NC._row_times4(xk[1], M[c, i, 1])
            xr = xs[at[N + R - 1]]
            f.append(TR.fma(prior[3], xr[:, 3], TR.fma(prior[2], xr[:, 2], TR.fma(prior[1], xr[:, 1], prior[0] * xr[:, 0]))))
        lg = np.log(RR._mix(w, np.array(f), True))
    return float(np.sum(lg)), float(np.sum(np.abs(lg)))


def measure_deep_rates(mp, child, blen, Q, prior, g, rates, weights):
    """treenni_cases.measure_deep under a mixture: (worst error of delta over EVERY move in units of (S + sum_s |d_s|) 2^-53; worst
    summed error of loglik + delta and of the restated mixture log-likelihood of apply_nni's tree against that tree's 50-digit
    value, over move_sample, in units of (S + sum_s |log m_s| + sum_s |log m'_s|) 2^-53; moves seen; impossible neighbours among
    them).  An impossible neighbour must be -inf in the restatement, and -inf as an explicit tree too."""
    S = g.shape[1]
    worst_n = worst_x = 0.0
    seen = dead_seen = 0
    for c, b in zip(child, blen):
        memo, rmemo, checked = {}, {}, False
        M = category_matrices(Q, b, rates)
        ll, delta, absd = RR.tree_nni_rates(c, M, prior, g, rates, weights)
        ell, eal, emv = RC.mp_tree_rates(mp, c, M, prior, g, weights)
        assert set(emv) == set(nni_moves(c))
        assert np.isnan(delta).sum() == delta.size - len(emv)
        l0, a0 = RC.mp_loglik_rates(mp, c, M, prior, g, weights, memo)
        assert abs(l0 - ell) < mp.mpf(10) ** -40 and abs(a0 - eal) < mp.mpf(10) ** -40
        picked = set(NC.move_sample(c))
        for (r, sd), (ed, ea, dead) in emv.items():
            seen += 1
            if dead:
                dead_seen += 1
                assert delta[r, sd] == -np.inf, (r, sd)
            else:
                assert np.isfinite(delta[r, sd]), (r, sd)
                assert abs(float(ea) - absd[r, sd]) <= 1e-9 * (1 + absd[r, sd])
                worst_n = max(worst_n, float(abs(mp.mpf(float(delta[r, sd])) - ed) / ((S + ea) * mp.mpf(2) ** -53)))
            if (r, sd) not in picked:
                continue
            c2, b2 = apply_nni(c, b, r, sd)
            M2 = np.array([NC.matrices_of(b2, b, M[k]) for k in range(len(weights))])
            ll2, _ = restated_loglik_rates(c2, M2, prior, g, weights, rmemo)
            if not checked:                                               # once per tree: the shared partials change no bit
                assert ll2 == RR.tree_loglik_sites(c2, M2, prior, g, weights)[0] or dead
                checked = True
            ell2, eal2 = RC.mp_loglik_rates(mp, c2, M2, prior, g, weights, memo)
            if dead:
                assert ll2 == -np.inf and ell2 == -mp.inf, (r, sd)
                continue
            assert abs(ell2 - (ell + ed)) < mp.mpf(10) ** -40, (r, sd)    # the move IS that tree
            unit = (S + eal + eal2) * mp.mpf(2) ** -53
            both = float((abs(mp.mpf(float(ll + delta[r, sd])) - ell2) + abs(mp.mpf(ll2) - ell2)) / unit)
            worst_x = max(worst_x, both)
    return worst_n, worst_x, seen, dead_seen


def per_tree_mixtures():
    """(rates [5][5], weights [5][5]): five different +I+G4 mixtures, one per tree of a big case"""
    mixes = [R.rate_model(a, 4, p, keep_invariant=True) for a, p in zip((0.2, 0.5, 1.0, 2.0, 5.0), (0.05, 0.1, 0.2, 0.02, 0.3))]
    return np.array([m[0] for m in mixes]), np.array([m[1] for m in mixes])


# ---- C. a workgroup's second item: the C-dependent cap of ptnr_updown's grid -------------------------------------------------------
T_SECOND = {5: 28, 16: 11}                                                 # trees of 512 taxa per mixture size: 3 past the cap
SAMPLE_SECOND = {5: [0, 1, 2, 12, 24, 25, 26, 27], 16: [0, 7, 8, 9, 10]}   # first items, a middle one, every second item


def rates_cap(N, C, cus):
    """ptnr_make_plan's cap on the grid of ptnr_updown, the items apart: min(8 CUs, 256 MiB / (C (N-1) U 2 KiB)), U = 2, at least 1"""
    return max(1, min(8 * cus, (256 << 20) // (C * (N - 1) * 2 * 2048)))


# ---- the restatement with the neighbours' site values kept -------------------------------------------------------------------------
def tree_values(child, M, prior, g, weights):
    """one tree, M [C][N-1][2][4][4]: (m [S], f [C][S], {move: m' [S]}, {move: f' [C][S]}) by treenni_rates_ref's own pieces"""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        per = [RR.category_factors(child, M[c], prior, g) for c in range(w.size)]
        f = np.array([p[0] for p in per])
        fp = {key: np.array([p[1][key] for p in per]) for key in per[0][1]}
        return RR._mix(w, f, True), f, {key: RR._mix(w, v, True) for key, v in fp.items()}, fp


def restated(child, M, prior, g, rates, weights, exact_mix=True):
    """T trees, M [T][C][N-1][2][4][4], rates and weights [C]: loglik [T], delta, absd [T][N-1][2], m [T][S].  exact_mix False (the
    512-taxon sets, a thousand moves a tree): the mixing chain by treegrad_ref.fma over whole arrays, the same bits inside fma's
    range (|w f| > 1e-290); the 512-taxon sets keep m above 2^-820, where a term outside that range is 2^-140 of m"""
    res = [RR.tree_nni_rates(c, m, prior, g, rates, weights, exact_mix=exact_mix, want_sites=True) for c, m in zip(child, M)]
    return tuple(np.array([r[k] for r in res]) for k in range(4))


# ---- D. the floor: delta where a category's factor of a neighbour is subnormal beside an m in range -------------------------------
FLOOR_MIXES = {'I+G4': MIX_I_G4, 'slow-fast': GC.MIX_SLOW_FAST}
FLOOR_RUNS = [(p, 'I+G4') for p in EC.PLACES] + [('at-the-floor', 'slow-fast')]


# The floor rule guards 1 / m, not a neighbour's own value m'.  Beside an m in [2^-1020, 2^-1000) a category's factor f'_c of a
# neighbour -- and m' itself where the neighbour is the less likely tree -- is subnormal, and a subnormal's rounding is absolute:
# half the smallest subnormal, 2^-1075, per operation.  Counted in ptnr_fold and pk_site_lik, not fitted, as section 13b counted
# K_W: with every factor at most 1 (leaves, matrix entries, messages, outer partials: abar_root is the prior and
# abar_child[k] = sum_j M[k][j] abar_p[j] msg[j] <= max_j abar_p[j]) one rounding of 2^-1075 reaches f'_c with a factor at most 1 from
#    pk_site_lik(av, xp): one product and three fma                                                    4
#    xp[j] = t[j] my[j]: one rounding per component, entering with av[j] <= 1                           4
#    t = pt2_row_times(xv, Mv): one product and three fma per component, entering with av[j] my[j]     16
#    xv[k] = mz[k] mc[k]: one rounding per component, entering with sum_j Mv[k][j] my[j] av[j] <= 1     4
# K_NNI = 28 roundings at the factor's own scale per category, and m' = w_0 f'_0, fma(w_c, f'_c, m') has weights at most 1.  So
# one neighbour's m'_s carries at most K_NNI C_live 2^-1075 (C_live the categories of positive weight), d_s = log(m'_s / m_s) that
# over m'_s, and the bound of one move is floor_allowance below on top of TOL_NNI_RATES (S + sum_s |d_s| + |value|).  What feeds
# these chains from the messages below and the outer partial above is rounded at the same scale and is NOT counted.
# Measured by test_treenni_rates_edges_cpu.py::test_near_floor_contract (restatement, scaled against unscaled, every in-range place,
# both mixtures, emulated and correctly rounded fma): the worst |difference| / allowance is 0.71 (FLOOR_WORST_RATIO; at-the-floor
# under MIX_SLOW_FAST, where the smallest m' is 2^-1021.0 and 738 category factors of neighbours are subnormal), and the SAME
# differences are 0.21 units of (S + sum_s |d_s| + |value|) 2^-53 at most (FLOOR_PLAIN_UNITS) where TOL_NNI_RATES is 23.2 of them:
# delta sums S = 130 sites, so its unit is 130 times a site's, and four sites' absolute errors of 2^-48 of themselves stay two
# orders of magnitude inside it.  So the device tests use NO allowance: near the floor delta is held to plain TOL_NNI_RATES,
# against the restatement on the scaled alignment (under hardware_fma) and against the unscaled call.  The whole allowance of these
# cases, 28 5 2^-1075 / 2^-1022.6 per site, is itself below the plain tolerance.  At 2^-900 and `inside` every entry of the
# restatement keeps the unscaled bits.
K_NNI = 28
FLOOR_WORST_RATIO = 0.71
FLOOR_PLAIN_UNITS = 0.21


def floor_allowance(mp_scaled, c_live, k=K_NNI):
    """sum_s k c_live 2^-1075 / m'_s over one neighbour's values at the scaled sites.  2^-1075 is below the smallest subnormal, so
    the unit is written as treegrad_edges_cases.floor_excess writes it: 2^-55 / (m' 2^1020)."""
    return float((k * c_live * 2.0 ** -55 / (np.asarray(mp_scaled, dtype=np.float64) * 2.0 ** 1020)).sum())


# ---- D. coded leaves: random columns reach the floor of m between 390 and 400 taxa ------------------------------------------------
# trees_edges_cases.random_columns(N) for N = 300, 310, ... 400 under MIX_I_G4 (test_treenni_rates_edges_cpu.py runs the search):
# the fast category keeps m well above the one-rate factor, which leaves the range at 310 taxa.  Tree 0's smallest m is 2^-984 at
# 380 taxa, 2^-1015.5 at 390 -- in range, beside subnormal category factors -- and 2^-1044 at 400, with 5 values below the floor
# and none zero: N = 400 is the smallest at which tree 0 leaves the range.  At 390 tree 2 already has two values below the floor
# (2^-1034) while trees 0 and 1 stay: the last N at which tree 0 stays in range is a set in which one tree is spoilt alone.
N_COLUMNS_IN, N_COLUMNS_OUT = 390, 400
