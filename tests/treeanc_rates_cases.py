"""Shared numbers and inputs of the tests of phylo_trees_ancestral_rates: the worst error of the NumPy
restatement (treeanc_rates_ref.py) against the same formulas at 50 digits, which sets the device tolerance; the near-floor
allowance, counted in the code; the restatement's worst row sums; the cases the device file runs, which the CPU file holds to
their preconditions first."""
import functools

import numpy as np

import treeanc_cases as AC
from phylo_amd import rates as R
from treeanc_cases import MAX_EXCLUDED, PRIOR, TINY  # noqa: F401
from treegrad_rates_cases import MIX_I_G4, category_matrices  # noqa: F401

# Measured by test_treeanc_rates_cpu.py::test_reference_against_mpmath (section 15's recipe under MIX_I_G4: N = 5, S = 8, gaps, 20
# trees, a GTR-like Q and JC69; p_inv = 0.1 + Gamma4(alpha = 0.5), so sites with f_0 = 0 are among them) before the kernel ran: the
# worst |reference - 50-digit value| in units of |value| 2^-53 (every term is non-negative, nothing cancels: the unit is the value
# itself).  Measured: post 6.90, catpost 6.86, siterate 3.65 (304 of the 320 tree-sites have f_0 = 0).  The test asserts that each
# stays at or below its constant here and above half of it.
E_REF_POST = 7.0
E_REF_CAT = 6.9
E_REF_RATE = 3.7
E_REF_ANC_RATES = max(E_REF_POST, E_REF_CAT, E_REF_RATE)
TOL_ANC_RATES = 8 * E_REF_ANC_RATES * 2.0 ** -53     # device against reference: |difference| <= TOL_ANC_RATES max(|reference|, TINY)

# Measured there too, over the same cases: the restatement's worst |sum_j post_j - 1| is 6 * 2^-53 and its worst
# |sum_c catpost_c - 1| is 2 * 2^-53 (neither is renormalised); held at 8 times that.
SUM_ERR_POST = 6 * 2.0 ** -53
SUM_ERR_CAT = 2 * 2.0 ** -53
SUM_TOL_POST = 8 * SUM_ERR_POST
SUM_TOL_CAT = 8 * SUM_ERR_CAT

# Above 128 taxa (section 13b's recipe: tree 0 of the case at four sites -- the first, the last and the first two variable ones
# between them), measured by test_treeanc_rates_cpu.py::test_reference_against_mpmath_big, same units, net of the absolute
# allowance below (a category whose own terms are subnormal beside an m in range, section 13b's finding):
#                                    post   catpost  siterate
#   caterpillar-N512   (C16)        62.02   42.69    1.40     (catpost raw: 2^53 -- a subnormal f_c the restatement holds as 0)
#   balanced-N512      (C16)        12.10   47.91    1.42     (the same)
#   balanced-N129-S130 (MIX_I_G4)    8.16   21.47    1.14
# The error grows with the depth of the tree, as sections 13b's and 14's did.  The test asserts that each case stays at or below
# its constant here and above half of it.
E_REF_BIG = {'caterpillar-N512': 62.1, 'balanced-N512': 48.0, 'balanced-N129-S130': 21.5}


def tol_big(name):
    return 8 * max(E_REF_ANC_RATES, E_REF_BIG[name]) * 2.0 ** -53


# ---- the near-floor allowance: counted in the code, not measured ---------------------------------------------------------------------
# The floor rule guards 1 / m, not a category's own terms.  Where m lies in [2^-1020, 2^-1000) -- or wherever a category's share of
# the site is so small that its own terms are subnormal beside an m in range -- a rounding is absolute: 2^-1075, half the smallest
# subnormal, per operation, whatever the value's size.  Per entry of a site's column, with d = 2^-1075 / m_s:
#   post[j]:  per category el[j] er[j] (one rounding), abar[j] * that (one more; abar[j] <= 1, so the first enters at most whole),
#             both carried by w_c, then w_c * q (one, not carried by w_c); the sums acc + w q of numbers below 2^-1022 are exact.
#             k_post = 2 sum_c w_c + C.
#   catpost_c: pk_site_lik's K_W = 5 roundings on f_c (section 13b), carried by w_c, and w_c * f_c (one).  k_cat = 5 w_c + 1.
#   siterate: sum_c r_c catpost_c, every product and sum at the size of the result.  k_rate = sum_c r_c (5 w_c + 1).
# As in section 13b what feeds these chains from further down the tree is rounded at the same scale and is NOT counted;
# test_treeanc_rates_cpu.py::test_near_floor_allowance prints the share of the bound the restatement uses.
def k_post(rates, weights):
    return 2.0 * float(np.sum(weights)) + len(weights)


def k_cat(rates, weights):
    return 5.0 * np.asarray(weights, dtype=np.float64) + 1.0


def k_rate(rates, weights):
    return float(np.sum(np.asarray(rates) * k_cat(rates, weights)))


def allowance(m, rates, weights):
    """(post [...][S], catpost [...][C][S], siterate [...][S]): k 2^-1075 / m_s for m [...][S]; 2^-1075 is below the smallest
    subnormal, so the unit is written as 2^-55 / (m 2^1020).  NaN sites (m below the floor): no allowance needed, NaN is compared as NaN."""
    with np.errstate(all='ignore'):
        d = 2.0 ** -55 / (np.asarray(m, dtype=np.float64) * 2.0 ** 1020)
    d = np.where(np.isfinite(d), d, 0.0)
    return k_post(rates, weights) * d, k_cat(rates, weights)[:, None] * d[..., None, :], k_rate(rates, weights) * d


def within(got, ref, extra=0.0, tol=None):
    """|got - ref| <= tol max(|ref|, TINY) + extra (tol: TOL_ANC_RATES); NaN against NaN passes.  Returns (ok [...], the worst
    error in units of the bound)"""
    tol = TOL_ANC_RATES if tol is None else tol
    with np.errstate(invalid='ignore'):
        bound = tol * np.maximum(np.abs(ref), TINY) + extra
        err = np.where(np.isnan(ref) & np.isnan(got), 0.0, np.abs(got - ref) / bound)
        err = np.where(np.isnan(err), np.inf, err)
    return err <= 1.0, float(err.max()) if err.size else 0.0


def decided(p, axis=-1):
    """bool: the two largest of p along `axis` differ by more than 2 TOL_ANC_RATES relative to the largest (one value only: decided)"""
    p = np.moveaxis(np.asarray(p), axis, -1)
    if p.shape[-1] == 1:
        return np.ones(p.shape[:-1], dtype=bool)
    with np.errstate(invalid='ignore'):
        top = np.sort(p, axis=-1)
        return (top[..., -1] - top[..., -2]) > 2 * TOL_ANC_RATES * top[..., -1]


# ---- the mixtures and the cases of the device file --------------------------------------------------------------------------------------
MIXTURES = {
    'C1': (np.array([1.0]), np.array([1.0])),
    'C2': (np.array([0.5, 1.5]), np.array([0.4, 0.6])),
    'C3z': (np.array([0.2, 1.0, 2.5]), np.array([0.5, 0.0, 0.5])),          # one zero weight
    'C5': MIX_I_G4,                                                          # +I+G4: the rate-0 category
    'C16': R.rate_model(0.7, 15, 0.05),
}
T_SMALL = 7                          # three chunks of PHYLO_TREES_CHUNK = 3


def case(N, S, mix, **kw):
    return dict(N=N, S=S, mix=mix, **kw)


# the smallest shapes at which the kernel can still go wrong: N = 2 (root only, no store), 3, 5, 12; S = 1, 63, 64, 65, 129, 130 in
# tiles of 64 (one to three tiles) and, under the default tile, a second site step with dead lanes; every mixture at least twice
CASES = {
    'N2-S1-C1': case(2, 1, 'C1', tile=64),
    'N2-S130-C5-gaps': case(2, 130, 'C5', tile=64, gaps=True),
    'N2-S64-C16-jc': case(2, 64, 'C16', tile=64, jc=True),
    'N3-S63-C2': case(3, 63, 'C2', tile=64),
    'N3-S65-C16-generic': case(3, 65, 'C16', tile=64, generic=True),
    'N3-S1-C5': case(3, 1, 'C5', tile=64),
    'N5-S64-C3z-jc': case(5, 64, 'C3z', tile=64, jc=True),
    'N5-S129-C5-gaps': case(5, 129, 'C5', tile=64, gaps=True),
    'N5-S130-C1-gaps-step2': case(5, 130, 'C1', gaps=True),                 # default tile: a strip of two steps, then one with 2 live lanes
    'N5-S65-C2-step2': case(5, 65, 'C2'),                                    # default tile: the second step has one live lane
    'N12-S130-C5-gaps': case(12, 130, 'C5', tile=64, gaps=True),
    'N12-S65-C3z-generic-step2': case(12, 65, 'C3z', generic=True),
    'N12-S129-C2-jc': case(12, 129, 'C2', tile=64, jc=True),
    'N12-S63-C16': case(12, 63, 'C16', tile=64),
}


def case_inputs(name):
    """(g, Q, child, blen, jc, tile, rates, weights) of a case, built by test_gpu_trees_loglik's own helpers"""
    from oracle import cpu_ref as O
    from test_gpu_trees_loglik import alignment, gtr_Q, random_trees
    kw = CASES[name]
    N, S, jc = kw['N'], kw['S'], kw.get('jc', False)
    g = alignment(N, S, 300 + N + S, kw.get('gaps', False), kw.get('generic', False))
    Q = O.jc_Q() if jc else gtr_Q()
    child, blen = random_trees(N, 6, T_SMALL)
    rates, weights = MIXTURES[kw['mix']]
    return g, Q, child, blen, jc, kw.get('tile'), rates, weights


@functools.lru_cache(maxsize=None)
def big_case(name):
    """(g, child, blen, Q, rates, weights, tile) of the cases above 128 taxa: trees_edges_cases' 512-taxon sets of five trees at
    S = 65 under 16 categories (32 MiB of node store per workgroup: 8 workgroups for the 10 items of tiles of 64), and
    test_gpu_treeanc's 129-taxon tree at S = 130 under MIX_I_G4"""
    import trees_edges_cases as EC
    if name == 'balanced-N129-S130':
        from test_gpu_treeanc import many_taxa_tree
        g, child, blen, Q = many_taxa_tree(129)
        return (g, child, blen, Q) + MIX_I_G4 + (64,)
    g, child, blen, Q = EC.big_case(name)
    return (g, child, blen, Q) + MIXTURES['C16'] + (64,)


def measure_big(mp, name):
    """the worst |restatement - 50-digit value| of post, catpost and siterate of tree 0 at the case's four sites
    (treegrad_edges_cases.mp_sites), in units of |value| 2^-53, net of the absolute allowance; and the same raw"""
    import treeanc_rates_ref as ARR
    from treegrad_edges_cases import mp_sites
    mpf = mp.mpf
    g, child, blen, Q, rates, weights, _ = big_case(name)
    c, b = child[0], blen[0]
    gs = np.ascontiguousarray(g[:, mp_sites(g)])
    M = category_matrices(Q, b, rates)
    ref = ARR.tree_ancestral_rates(c, M, PRIOR, gs, rates, weights)
    assert np.isfinite(ref['post']).all() and (ref['m'] >= AC.TINY).all()
    return measure(mp, c, M, gs, rates, weights, ref)


def measure(mp, c, M, gs, rates, weights, ref, prior=PRIOR):
    mpf = mp.mpf
    cv = lambda a: [cv(v) for v in a] if np.ndim(a) else mpf(float(a))
    Mm, pm, rm, wm = cv(M), cv(prior), cv(rates), cv(weights)
    N, S, C = gs.shape[0], gs.shape[1], len(rates)
    worst = {'post': 0.0, 'catpost': 0.0, 'siterate': 0.0, 'post_raw': 0.0, 'catpost_raw': 0.0, 'siterate_raw': 0.0}
    kp, kc, kr = k_post(rates, weights), k_cat(rates, weights), k_rate(rates, weights)

    def err(key, val, exact, k, d):
        if exact == 0:
            assert val == 0.0, (key, val)
            return
        unit = abs(exact) * mpf(2) ** -53
        diff = abs(mpf(float(val)) - exact)
        worst[key + '_raw'] = max(worst[key + '_raw'], float(diff / unit))
        over = diff - mpf(float(k)) * d
        if over > 0:
            worst[key] = max(worst[key], float(over / unit))

    for s in range(S):
        m, post, catpost, siterate, f = ARR_site(c.tolist(), Mm, pm, cv(gs[:, s]), rm, wm, mpf(0))
        d = mpf(2) ** -1075 / m
        for i in range(N - 1):
            for j in range(4):
                err('post', ref['post'][i, s, j], post[i][j], kp, d)
        for k in range(C):
            err('catpost', ref['catpost'][k, s], catpost[k], kc[k], d)
        err('siterate', ref['siterate'][s], siterate, kr, d)
    worst['subnormal_f'] = int(((ref['f'] > 0) & (ref['f'] < 2.0 ** -1022)).sum())
    return worst


def ARR_site(*a):
    import treeanc_rates_ref as ARR
    return ARR.site_terms_rates(*a)
